#!/usr/bin/env python3
"""Renders a scene to the 8-bit quilt PNG and the interlaced PNG of a lenticular display.

    python tools/quilt_display.py [scene.xml] [-D key=value ...] [--preset NAME --presets presets.csv]
                                  [--size W H] [--nearest] [--out-dir DIR] [--depth PATH]
                                  [--denoise [ITER]] [--temporal N [--denoise-variance]] [--synth GX GY]
                                  [--tonemap {linear,reinhard,aces}] [--ev X] [--auto-exposure] [--adapt A]

Without arguments: scenes/cbox_grid.xml at a small resolution, the default preset (LKG4x8) with the scene's view
grid, a 1280 x 720 display, written to out/<scene>_quilt.png and out/<scene>_display.png.  The frame is rendered once;
both images come from that frame.  --depth PATH also writes the depth quilt (nearer brighter, background black, scaled to
the frame's own depth range) as an 8-bit PNG: the RGB-D companion of the quilt.  --denoise [ITER] filters the developed
frame on the device before both images are made (amvpt.denoise's defaults; ITER iterations instead of 3).  --temporal N
renders N frames at the given spp with consecutive seeds through an amvpt.TemporalAccumulator and shows the last one
(with --denoise, filtered after the accumulation).  --temporal N --denoise-variance filters with the variance-guided
denoiser of include/amvpt_variance.h instead: the accumulator carries the luminance moments, and the filter is as wide as
the variance they give (amvpt.VarianceParams' defaults, sigma_plane scaled to the scene).  --synth GX GY loads the scene
a second time with gx=GX gy=GY and shows that denser quilt, synthesized from the rendered one without tracing a path
(amvpt.ViewSynthesizer, include/amvpt_synth.h; after --denoise where given), and prints how many holes are left.
--tonemap OP, --ev X, --auto-exposure and --adapt A (any of them) put an amvpt.ToneMapper (include/amvpt_tonemap.h) in
the place of the sRGB conversion of both images: the operator OP (default linear), X stops of exposure compensation, the
exposure metered from the quilt's histogram instead of fixed, and the share A of the gap in log2 exposure closed per frame
(with --temporal; default 1).  The exposure used is printed.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mitsuba3-amvpt_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default=os.path.join(REPO, "scenes", "cbox_grid.xml"))
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="key=value")
    ap.add_argument("--presets", help="a presets.csv to take --preset from")
    ap.add_argument("--preset", help="name of a preset in --presets (default: LKG4x8 with the scene's grid)")
    ap.add_argument("--size", type=int, nargs=2, default=(1280, 720), metavar=("W", "H"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--nearest", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "out"))
    ap.add_argument("--depth", metavar="PATH", help="also write the depth quilt (amvpt.display.depth_quilt) as a PNG")
    ap.add_argument("--denoise", type=int, nargs="?", const=3, default=None, metavar="ITER",
                    help="filter the frame with the a-trous denoiser (amvpt.denoise), ITER iterations (default 3)")
    ap.add_argument("--temporal", type=int, default=None, metavar="N",
                    help="accumulate N frames of consecutive seeds (amvpt.TemporalAccumulator) and show the last")
    ap.add_argument("--denoise-variance", action="store_true",
                    help="with --temporal: filter with the variance-guided denoiser (amvpt.VarianceParams' defaults)")
    ap.add_argument("--synth", type=int, nargs=2, default=None, metavar=("GX", "GY"),
                    help="show the GX x GY quilt of the same scene, synthesized from the rendered views (amvpt.ViewSynthesizer)")
    ap.add_argument("--tonemap", choices=("linear", "reinhard", "aces"), default=None,
                    help="tone-map with this operator (amvpt.ToneMapper) instead of clipping at 1")
    ap.add_argument("--ev", type=float, default=None, metavar="X", help="exposure compensation in stops")
    ap.add_argument("--auto-exposure", action="store_true", help="meter the exposure from the quilt's log-luminance histogram")
    ap.add_argument("--adapt", type=float, default=None, metavar="A",
                    help="with --auto-exposure: the share of the gap in log2 exposure closed per frame (default 1)")
    a = ap.parse_args()
    if a.denoise_variance and (a.temporal is None or a.denoise is not None):
        ap.error("--denoise-variance needs --temporal and excludes --denoise")
    if a.synth is not None and a.temporal is not None:
        ap.error("--synth excludes --temporal")

    import amvpt
    import amvpt.display as D

    defines = dict(d.split("=", 1) for d in a.defines)
    if os.path.basename(a.scene) == "cbox_grid.xml" and not a.defines:
        defines = dict(res=128, gx=4, gy=2, spp=16)
    scene = amvpt.load_file(a.scene, **defines)
    preset = None
    if a.preset:
        if not a.presets:
            ap.error("--preset needs --presets")
        found = [p for p in D.read_presets(a.presets) if p.name == a.preset]
        if not found:
            ap.error("no preset %r in %s" % (a.preset, a.presets))
        preset = found[-1]
    w, h, _, _ = scene.film_info()
    cnt = amvpt.Counters()
    # one render; the 8-bit quilt from its download (the host entry gives the device's bytes), the display image
    # from the stage run on the frame the render left on the device
    a.tm = None
    if a.tonemap is not None or a.ev is not None or a.auto_exposure or a.adapt is not None:
        a.tm = amvpt.ToneMapper(amvpt.TonemapParams(op=a.tonemap or "linear", auto_exposure=a.auto_exposure, ev=a.ev or 0.0,
                                                    adapt=1.0 if a.adapt is None else a.adapt))
    if a.temporal is not None:
        return temporal_frames(a, ap, scene, preset, cnt)
    if a.synth is not None:
        return synthesized(a, scene, defines, preset, cnt)
    if a.tm is not None:
        return tone_mapped(a, scene, preset, cnt)
    frame = amvpt.render(scene, seed=a.seed, spp=a.spp, counters=cnt)
    if a.denoise is not None:   # the filtered frame replaces the cached one: the display image below shows it
        q = amvpt.denoise_params_for(scene, iterations=a.denoise)
        frame = amvpt.host_denoise(scene, q, replace=True)
    quilt = D.srgb8(frame)
    image = D.display(scene, preset, size=tuple(a.size), nearest=a.nearest, rerender=False)
    os.makedirs(a.out_dir, exist_ok=True)
    stem = os.path.join(a.out_dir, os.path.splitext(os.path.basename(a.scene))[0])
    D.write_png(stem + "_quilt.png", quilt)
    D.write_png(stem + "_display.png", image)
    if a.depth:
        D.write_png(a.depth, D.depth_quilt(scene))
    used = preset if preset is not None else D.preset_for_scene(scene)
    print("%s: quilt %d x %d -> %s_quilt.png, display %d x %d (%s, grid %d x %d) -> %s_display.png, %d lanes" % (
        os.path.basename(a.scene), w, h, stem, a.size[0], a.size[1], used.name, used.grid[0], used.grid[1], stem,
        cnt.lanes))


def quilt8(a, frame):
    """The 8-bit quilt of the float frame shown last (a device tensor): clipped, or as the tone mapper left it."""
    import amvpt
    import amvpt.display as D
    if a.tm is None:
        return D.srgb8(frame.cpu().numpy())
    s = a.tm.state()
    print("tone mapping: %s, exposure %.6g%s" % (
        a.tonemap or "linear", s.exposure if a.tm.params.auto_exposure else 2.0 ** a.tm.params.ev,
        " (metered over %d pixels, %d skipped)" % (s.counted, s.skipped) if a.tm.params.auto_exposure else ""))
    return amvpt.tonemap_srgb8_host(frame.cpu().numpy(), a.tm.params, state=s)


def tone_mapped(a, scene, preset, cnt):
    """A tone mapper and neither --temporal nor --synth: one display over torch tensors; the quilt is its frame."""
    import amvpt
    import amvpt.display as D
    denoise = amvpt.denoise_params_for(scene, iterations=a.denoise) if a.denoise is not None else None
    image = D.display(scene, preset, size=tuple(a.size), nearest=a.nearest, seed=a.seed, spp=a.spp, counters=cnt, denoise=denoise,
                      tonemap=a.tm)
    os.makedirs(a.out_dir, exist_ok=True)
    stem = os.path.join(a.out_dir, os.path.splitext(os.path.basename(a.scene))[0])
    D.write_png(stem + "_quilt.png", quilt8(a, a.tm.frame))
    D.write_png(stem + "_display.png", image)
    if a.depth:
        D.write_png(a.depth, D.depth_quilt(scene))
    print("%s: tone-mapped quilt -> %s_quilt.png, %s_display.png, %d lanes" % (os.path.basename(a.scene), stem, stem, cnt.lanes))


def temporal_frames(a, ap, scene, preset, cnt):
    """--temporal N: N displays through one accumulator; the quilt is the accumulator's last image."""
    import amvpt
    import amvpt.display as D
    if a.temporal < 1:
        ap.error("--temporal needs at least one frame")
    acc = amvpt.TemporalAccumulator(moments=a.denoise_variance)
    denoise = amvpt.denoise_params_for(scene, iterations=a.denoise) if a.denoise is not None else None
    if a.denoise_variance:
        denoise = amvpt.VarianceParams(sigma_plane=amvpt.denoise_params_for(scene).sigma_plane)
    for i in range(a.temporal):
        image = D.display(scene, preset, size=tuple(a.size), nearest=a.nearest, seed=a.seed + i, spp=a.spp, counters=cnt,
                          denoise=denoise, temporal=acc, tonemap=a.tm)
    os.makedirs(a.out_dir, exist_ok=True)
    stem = os.path.join(a.out_dir, os.path.splitext(os.path.basename(a.scene))[0])
    D.write_png(stem + "_quilt.png", quilt8(a, acc.image if a.tm is None else a.tm.frame))
    D.write_png(stem + "_display.png", image)
    if a.depth:
        D.write_png(a.depth, D.depth_quilt(scene))
    print("%s: %d frames accumulated (mean history %.2f) -> %s_quilt.png, %s_display.png" % (
        os.path.basename(a.scene), a.temporal, float(acc.count.mean()), stem, stem))


def synthesized(a, scene, defines, preset, cnt):
    """--synth GX GY: one display through a ViewSynthesizer; the quilt is the synthesizer's dense image."""
    import amvpt
    import amvpt.display as D
    dense = amvpt.load_file(a.scene, **dict(defines, gx=a.synth[0], gy=a.synth[1]))
    vs = amvpt.ViewSynthesizer(dense)
    denoise = amvpt.denoise_params_for(scene, iterations=a.denoise) if a.denoise is not None else None
    image = D.display(scene, preset, size=tuple(a.size), nearest=a.nearest, seed=a.seed, spp=a.spp, counters=cnt, denoise=denoise,
                      synth=vs, tonemap=a.tm)
    os.makedirs(a.out_dir, exist_ok=True)
    stem = os.path.join(a.out_dir, os.path.splitext(os.path.basename(a.scene))[0])
    D.write_png(stem + "_quilt.png", quilt8(a, vs.image))
    D.write_png(stem + "_display.png", image)
    if a.depth:
        D.write_png(a.depth, D.depth_quilt(dense))
    w, h = int(vs.dst_params.film_width), int(vs.dst_params.film_height)
    print("%s: %d views synthesized from %d rendered ones, quilt %d x %d, %d holes of %d pixels (%d filled) -> %s_quilt.png, "
          "%s_display.png" % (os.path.basename(a.scene), len(vs.dst_views), scene.describe(0, 0, 0)[2].n_views, w, h, vs.holes,
                              w * h, int((vs.cover < 0).sum().item()), stem, stem))


if __name__ == "__main__":
    main()

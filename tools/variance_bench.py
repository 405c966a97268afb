#!/usr/bin/env python3
"""Times the launches of the variance-guided denoiser (amvpt_variance.h) on one GPU.

Default shape: the quilt of bench.py's config M (cbox_grid.xml, 4 x 2 views of 1024 x 1024: 4096 x 2048) with real
guide records and real frames.  The planes are what an accumulator holds after --frames frames of a camera that moves
by --shift world units a frame (amvpt.TemporalAccumulator(moments=True)); the last push's inputs are kept, so that
stage 1 is timed on a real history.  Timed, each with HIP events around single calls after warm-up calls, alternating
inside every repeat: amvpt_temporal_moments beside amvpt_temporal on the same planes, amvpt_variance, and every
iteration of amvpt_denoise_variance on its own (the call with iterations = 1 .. --iterations, differences of the
medians) beside amvpt_denoise at the same iteration counts.  min / median / max over the repeats, beside each launch's
byte floor and the fraction of the HBM peak that gives.  Prints one JSON object.

    python tools/variance_bench.py [--res 1024] [--gx 4 --gy 2] [--spp 1] [--frames 4] [--shift 0.02 0.01]
                                   [--iterations 4] [--repeats 20] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mitsuba3-amvpt_amd"))

HBM_PEAK_GBS = 8000.0   # MI355X: 8 TB/s
CAMERA = 'origin="0, 0, 3.9" target="0, 0, 0"'


def stats(ms, nbytes):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"min_ms": round(ms[0], 4), "median_ms": round(med, 4), "max_ms": round(ms[-1], 4),
            "floor_bytes": nbytes, "gb_per_s_at_median": round(nbytes / med / 1e6, 1),
            "hbm_fraction_at_median": round(nbytes / med / 1e6 / HBM_PEAK_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--gx", type=int, default=4)
    ap.add_argument("--gy", type=int, default=2)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--shift", type=float, nargs=2, default=(0.02, 0.01), metavar=("DX", "DY"))
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch

    import amvpt

    assert torch.cuda.is_available(), "variance_bench.py needs a GPU"
    assert a.frames >= 2
    L = amvpt.hip_lib()
    xml = open(os.path.join(REPO, "scenes", "cbox_grid.xml")).read()
    assert CAMERA in xml
    acc = amvpt.TemporalAccumulator(moments=True)
    dev = None
    for i in range(a.frames):
        dx, dy = a.shift[0] * (i - a.frames + 1), a.shift[1] * (i - a.frames + 1)
        s = amvpt.load_string(xml.replace(CAMERA, 'origin="%g, %g, 3.9" target="%g, %g, 0"' % (dx, dy, dx, dy)),
                              res=a.res, gx=a.gx, gy=a.gy, spp=a.spp, reuse=8)
        sd, vd, p = s.describe(0, i, a.spp)
        dev = dev or amvpt.DeviceScene(sd)
        w, h = p.film_width, p.film_height
        c = 4 if p.film_alpha else 3
        film = torch.zeros((h, w, c + 1), dtype=torch.float32, device="cuda")
        img = torch.empty((h, w, c), dtype=torch.float32, device="cuda")
        dev.render(vd, p, film.data_ptr())
        assert L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(img.data_ptr()), w, h, p.film_alpha, None) == 0
        if i == a.frames - 1:   # the history the last push reads: copies, since the push swaps the accumulator's sets
            hist = [t.clone() for t in (acc.image, acc.guides, acc.count, acc.moments)]
            prev_views = acc.prev_views
        acc.push(dev, vd, p, img)
        del film
    torch.cuda.synchronize()
    g, cnt, mom, frame = acc.guides, acc.count, acc.moments, acc.image
    npx = w * h
    q = amvpt.VarianceParams(iterations=a.iterations)
    var = acc.variance(q)
    out, scratch = torch.empty_like(frame), torch.empty_like(frame)
    vout, vscratch = torch.empty_like(var), torch.empty_like(var)
    o_img, o_cnt, o_mom = torch.empty_like(frame), torch.empty_like(cnt), torch.empty_like(mom)

    def temporal():
        amvpt.temporal_device(img.data_ptr(), c, g.data_ptr(), hist[0].data_ptr(), hist[1].data_ptr(), hist[2].data_ptr(), prev_views,
                              p, o_img.data_ptr(), o_cnt.data_ptr())

    def temporal_moments():
        amvpt.temporal_moments_device(img.data_ptr(), c, g.data_ptr(), hist[0].data_ptr(), hist[1].data_ptr(), hist[2].data_ptr(),
                                      hist[3].data_ptr(), prev_views, p, o_img.data_ptr(), o_cnt.data_ptr(), o_mom.data_ptr())

    def variance():
        amvpt.variance_device(mom.data_ptr(), cnt.data_ptr(), g.data_ptr(), w, h, vout.data_ptr(), params=q)

    def filter_at(n):
        qn = amvpt.VarianceParams(iterations=n)
        return lambda: amvpt.denoise_variance_device(frame.data_ptr(), c, w, h, var.data_ptr(), g.data_ptr(), out.data_ptr(),
                                                     scratch.data_ptr(), vout.data_ptr(), vscratch.data_ptr(), params=qn)

    def today_at(n):
        qn = amvpt.DenoiseParams(iterations=n)
        return lambda: amvpt.denoise_device(frame.data_ptr(), c, w, h, g.data_ptr(), out.data_ptr(), scratch.data_ptr(), qn)

    calls = {"amvpt_temporal": temporal, "amvpt_temporal_moments": temporal_moments, "amvpt_variance": variance}
    for n in range(1, a.iterations + 1):
        calls["amvpt_denoise_variance_%d" % n] = filter_at(n)
        calls["amvpt_denoise_%d" % n] = today_at(n)
    times = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):          # the calls alternate inside every repeat
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    f = 4
    floors = {"amvpt_temporal": npx * (2 * f * c + 2 * 32 + 4 + f * c + 4),
              "amvpt_temporal_moments": npx * (2 * f * c + 2 * 32 + 4 + 8 + f * c + 4 + 8),
              "amvpt_variance": npx * (8 + 4 + 4)}   # moments, count, out; the guides only where the history is short
    per_iteration = npx * (f * c + 4 + 32 + f * c + 4)   # image, variance, guides read; image, variance written
    res = {"quilt": [w, h], "channels": c, "spp": a.spp, "frames": a.frames, "shift": list(a.shift), "repeats": a.repeats,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_per_s": HBM_PEAK_GBS,
           "count_below_min_history": round(float((cnt < q.min_history).float().mean()), 4),
           "floor_bytes_per_filter_iteration": per_iteration}
    for name in calls:
        if name.startswith("amvpt_denoise_variance_"):
            nbytes = per_iteration * int(name.rsplit("_", 1)[1])
        elif name.startswith("amvpt_denoise_"):
            nbytes = npx * (2 * f * c + 32) * int(name.rsplit("_", 1)[1])
        else:
            nbytes = floors[name]
        res[name] = stats(times[name], nbytes)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

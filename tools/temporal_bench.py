#!/usr/bin/env python3
"""Times the temporal accumulation kernel (amvpt_temporal.h) on one GPU.

Default shape: the quilt of bench.py's config M (cbox_grid.xml, 4 x 2 views of 1024 x 1024: 4096 x 2048) with real
guide records and real 16-spp frames.  Two histories are timed, alternating inside every repeat: a second frame of
the same camera with another seed (`static`: every hit pixel reprojects into itself) and a frame of a camera shifted
by --shift world units (`shifted`: taps land some pixels away, a share of them is stopped).  Either history has
planes of its own, as the planes an accumulator keeps are: no history plane is one of the current frame's.  The
history planes are what a first accumulation of the previous frame leaves (count 1).  Each call is timed with HIP
events around it (the view-table upload and the one launch) after warm-up calls; min / median / max over the repeats,
beside the byte floor (108 B a pixel with 3 channels) and the fraction of the HBM peak that gives.  Prints one JSON
object.

    python tools/temporal_bench.py [--res 1024] [--gx 4 --gy 2] [--spp 16] [--shift 0.02 0.01] [--repeats 20] [--warmup 3]
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
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--shift", type=float, nargs=2, default=(0.02, 0.01), metavar=("DX", "DY"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch

    import amvpt

    assert torch.cuda.is_available(), "temporal_bench.py needs a GPU"
    L = amvpt.hip_lib()
    xml = open(os.path.join(REPO, "scenes", "cbox_grid.xml")).read()
    assert CAMERA in xml
    dx, dy = a.shift
    shifted = xml.replace(CAMERA, 'origin="%g, %g, 3.9" target="%g, %g, 0"' % (dx, dy, dx, dy))
    defines = dict(res=a.res, gx=a.gx, gy=a.gy, spp=a.spp, reuse=8)
    scenes = {"current": amvpt.load_string(xml, **defines), "static": amvpt.load_string(xml, **defines),
              "shifted": amvpt.load_string(shifted, **defines)}
    dev = None
    frames = {}
    for seed, (name, s) in enumerate(scenes.items()):
        sd, vd, p = s.describe(0, seed, a.spp)
        dev = dev or amvpt.DeviceScene(sd)
        w, h = p.film_width, p.film_height
        c = 4 if p.film_alpha else 3
        film = torch.zeros((h, w, c + 1), dtype=torch.float32, device="cuda")
        img = torch.empty((h, w, c), dtype=torch.float32, device="cuda")
        g = torch.empty((h, w, 8), dtype=torch.float32, device="cuda")
        dev.render(vd, p, film.data_ptr())
        assert L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(img.data_ptr()), w, h, p.film_alpha, None) == 0
        dev.guides(vd, p, g.data_ptr())
        frames[name] = (img, g, vd, p)
        del film
    torch.cuda.synchronize()
    img, g, vd, p = frames["current"]
    w, h = p.film_width, p.film_height
    c = img.shape[2]
    ones = torch.ones((h, w), dtype=torch.float32, device="cuda")
    out, cnt = torch.empty_like(img), torch.empty_like(ones)
    histories = {"static": frames["static"][:3], "shifted": frames["shifted"][:3]}
    for hi, hg, _ in histories.values():
        assert hi.data_ptr() != img.data_ptr() and hg.data_ptr() != g.data_ptr()

    def run(name):
        hi, hg, pv = histories[name]
        amvpt.temporal_device(img.data_ptr(), c, g.data_ptr(), hi.data_ptr(), hg.data_ptr(), ones.data_ptr(), pv, p,
                              out.data_ptr(), cnt.data_ptr())

    times = {k: [] for k in histories}
    accepted = {}
    for name in histories:
        for _ in range(a.warmup):
            run(name)
        torch.cuda.synchronize()
        hit = g[..., 0] >= 0
        accepted[name] = round(float(((cnt == 2) & hit).sum() / hit.sum()), 4)
    for _ in range(a.repeats):          # the histories alternate inside every repeat
        for name in histories:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    floor = w * h * (2 * 4 * c + 2 * 32 + 4 + 4 * c + 4)   # current image + guides, history, outputs
    res = {"quilt": [w, h], "channels": c, "spp": a.spp, "shift": [dx, dy], "repeats": a.repeats, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "hbm_peak_gb_per_s": HBM_PEAK_GBS,
           "hit_pixels_with_history": accepted}
    for name in histories:
        res[name] = stats(times[name], floor)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

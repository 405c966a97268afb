#!/usr/bin/env python3
"""Times the kernels of the view synthesis (amvpt_synth.h) on one GPU.

Default shape: cbox_grid.xml as 8 source views of 1024 x 1024 (config M's quilt, 4096 x 2048) synthesized into a
4096 x 2048 target quilt of 8 x 4 views of 512 x 512.  The guide records of both quilts come from amvpt_guides; the
source image is seeded noise (the kernels' work depends on the records, which decide every stop, not on the colours).
Timed with HIP events around single launches after warm-up launches, as tools/display_bench.py times its kernels, the
three alternating inside every repeat: stage 1 (k_synth), one fill iteration (k_synth_fill at step 1, on stage 1's
output) and amvpt_guides for the target quilt.  Per kernel min / median / max, the bytes it must move at least and the
fraction of the HBM peak that gives.  --frame-ms is the time of a rendered frame (bench.py's ms per step of the same
commit): the three together are reported as a fraction of it.  Prints one JSON object.

    python tools/synth_bench.py [--src 1024 4 2] [--dst 512 8 4] [--channels 3] [--repeats 20] [--warmup 3] [--frame-ms MS]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mitsuba3-amvpt_amd"))

HBM_PEAK_GBS = 8000.0   # MI355X: 8 TB/s


def stats(ms, nbytes):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"min_ms": round(ms[0], 4), "median_ms": round(med, 4), "max_ms": round(ms[-1], 4),
            "min_bytes": nbytes, "gb_per_s_at_median": round(nbytes / med / 1e6, 1),
            "hbm_fraction_at_median": round(nbytes / med / 1e6 / HBM_PEAK_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(REPO, "scenes", "cbox_grid.xml"))
    ap.add_argument("--src", type=int, nargs=3, default=(1024, 4, 2), metavar=("RES", "GX", "GY"))
    ap.add_argument("--dst", type=int, nargs=3, default=(512, 8, 4), metavar=("RES", "GX", "GY"))
    ap.add_argument("--channels", type=int, default=3, choices=(3, 4))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frame-ms", type=float, default=None, help="ms of a rendered frame, to report the stage's share of it")
    a = ap.parse_args()

    import torch

    import amvpt

    assert torch.cuda.is_available(), "synth_bench.py needs a GPU"
    src = amvpt.load_file(a.scene, res=a.src[0], gx=a.src[1], gy=a.src[2])
    dst = amvpt.load_file(a.scene, res=a.dst[0], gx=a.dst[1], gy=a.dst[2])
    sd, sv, sp = src.describe(0, 0, 0)
    _, dv, dp = dst.describe(0, 0, 0)
    dev = amvpt.DeviceScene(sd)
    hs, ws, h, w, c = sp.film_height, sp.film_width, dp.film_height, dp.film_width, a.channels
    gen = torch.Generator(device="cuda").manual_seed(1)
    image = torch.rand((hs, ws, c), dtype=torch.float32, device="cuda", generator=gen) + 0.01
    sg = torch.empty((hs, ws, 8), dtype=torch.float32, device="cuda")
    dg = torch.empty((h, w, 8), dtype=torch.float32, device="cuda")
    dev.guides(sv, sp, sg.data_ptr())
    out, cover = torch.empty((h, w, c), dtype=torch.float32, device="cuda"), torch.empty((h, w), dtype=torch.float32, device="cuda")
    fout, fcover = torch.empty_like(out), torch.empty_like(cover)
    q = amvpt.SynthParams(fill_iterations=1)

    def guides():
        dev.guides(dv, dp, dg.data_ptr())

    def stage1():
        amvpt.synth_device(image.data_ptr(), c, sg.data_ptr(), sv, sp, dg.data_ptr(), dv, dp, out.data_ptr(), cover.data_ptr(), sp=q)

    def fill():
        amvpt.synth_fill_device(out.data_ptr(), c, w, h, cover.data_ptr(), dg.data_ptr(), fout.data_ptr(), fcover.data_ptr(), sp=q)

    kernels = {"amvpt_guides": guides, "k_synth": stage1, "k_synth_fill": fill}
    times = {k: [] for k in kernels}
    for fn in kernels.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):          # the kernels alternate inside every repeat
        for name, fn in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    px = h * w
    nbytes = {"amvpt_guides": px * 32,                  # the records written once
              "k_synth": px * (32 + 4 * (c + 1)),       # the target records read once, image and cover written once
              "k_synth_fill": px * 8 * (c + 1)}         # image and cover read once and written once
    res = {"scene": os.path.basename(a.scene), "source": {"views": int(sp.n_views), "quilt": [int(ws), int(hs)]},
           "target": {"views": int(dp.n_views), "quilt": [int(w), int(h)]}, "channels": c, "repeats": a.repeats, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "hbm_peak_gb_per_s": HBM_PEAK_GBS,
           "holes_after_stage_1": int((cover == 0).sum().item()), "filled_by_one_iteration": int((fcover < 0).sum().item()),
           "mean_cover": round(float(cover.mean().item()), 4)}
    for name in kernels:
        res[name] = stats(times[name], nbytes[name])
    res["stage_median_ms"] = round(sum(res[k]["median_ms"] for k in kernels), 4)
    if a.frame_ms:
        res["frame_ms"] = a.frame_ms
        res["stage_fraction_of_frame"] = round(res["stage_median_ms"] / a.frame_ms, 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

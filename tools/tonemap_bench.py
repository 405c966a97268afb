#!/usr/bin/env python3
"""Times the kernels of the tone-mapping stage (amvpt_tonemap.h) on one GPU.

Default shape: cbox_grid.xml rendered as 8 views of 1024 x 1024, the 4096 x 2048 x 3 quilt of config M.  Timed with HIP
events around single calls after warm-up calls, as tools/synth_bench.py times its kernels, all alternating inside every
repeat: amvpt_srgb8 (k_srgb8, the step the stage replaces, as the baseline), amvpt_tonemap_meter (the fill of the counts,
k_tonemap_hist and k_exposure) on the rendered frame and on a frame whose pixels all fall in one bin (the worst
same-address contention), and amvpt_tonemap_srgb8 (k_tonemap writing bytes, the exposure read from the state) for each
operator.  Per call min / median / max, the bytes it must move at least and the fraction of the HBM peak that gives.
Prints one JSON object.

    python tools/tonemap_bench.py [--res 1024 4 2] [--spp 4] [--repeats 30] [--warmup 5]
"""
import argparse
import ctypes
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
    ap.add_argument("--res", type=int, nargs=3, default=(1024, 4, 2), metavar=("RES", "GX", "GY"))
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()

    import torch

    import amvpt
    import amvpt.display as D

    assert torch.cuda.is_available(), "tonemap_bench.py needs a GPU"
    scene = amvpt.load_file(a.scene, res=a.res[0], gx=a.res[1], gy=a.res[2], spp=a.spp)
    frame = torch.from_numpy(amvpt.render(scene, seed=1)).cuda().contiguous()
    h, w, c = (int(v) for v in frame.shape)
    flat = torch.full_like(frame, 0.5)
    q8 = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    state = torch.zeros(ctypes.sizeof(amvpt.TonemapState), dtype=torch.uint8, device="cuda")
    auto = {op: amvpt.TonemapParams(op=op, auto_exposure=True) for op in ("linear", "reinhard", "aces")}

    def srgb8():
        D.srgb8_device(frame.data_ptr(), c, w, h, q8.data_ptr())

    def meter(img):
        return lambda: amvpt.tonemap_meter_device(img.data_ptr(), c, w, h, state.data_ptr(), auto["linear"])

    def fused(op):
        return lambda: amvpt.tonemap_srgb8_device(frame.data_ptr(), c, w, h, q8.data_ptr(), auto[op], state_ptr=state.data_ptr())

    calls = {"k_srgb8": srgb8, "meter_one_bin": meter(flat), "meter_rendered": meter(frame)}
    calls.update({"k_tonemap_srgb8_" + op: fused(op) for op in auto})   # after meter_rendered: its exposure is the state's
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
    px = h * w
    s = amvpt.TonemapState.from_buffer_copy(state.cpu().numpy().tobytes())
    hist = s.histogram()
    res = {"scene": os.path.basename(a.scene), "quilt": [w, h], "channels": c, "spp": a.spp, "repeats": a.repeats,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_per_s": HBM_PEAK_GBS,
           "lib_dir": os.path.basename(amvpt.LIB_DIR),
           "rendered_frame": {"max": float(frame.max().item()), "counted": int(s.counted), "skipped": int(s.skipped),
                              "bins_used": int((hist > 0).sum()), "largest_bin_share": round(float(hist.max()) / max(1, px), 4),
                              "exposure": float(s.exposure)}}
    for name in calls:
        res[name] = stats(times[name], px * 4 * c if name.startswith("meter") else px * (4 * c + 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

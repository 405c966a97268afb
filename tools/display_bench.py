#!/usr/bin/env python3
"""Times the two kernels of the display stage (amvpt_display.h) on one GPU.

Default shape: an 8192 x 8192 quilt (4 x 8 views of 2048 x 1024) and a 7680 x 4320 display with the default preset.
Each kernel is timed with HIP events around single launches after warm-up launches, as DESIGN.md section 7 times
kernels; min / median / max over the repeats, the bytes the kernel must move at least (source read once plus
destination written once) and the fraction of the HBM peak that gives.  The dword-store instance of k_interlace is
alternated with the byte-store instance, which the library selects for a destination off dword alignment: the second
variant therefore also writes one byte off alignment, and the pair compares aligned dwords with misaligned bytes, not
store width alone.  Likewise k_srgb8's vector instance with its scalar one.  Prints one JSON object.

    python tools/display_bench.py [--quilt 8192 8192] [--size 7680 4320] [--repeats 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

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
    ap.add_argument("--quilt", type=int, nargs=2, default=(8192, 8192), metavar=("W", "H"))
    ap.add_argument("--size", type=int, nargs=2, default=(7680, 4320), metavar=("W", "H"))
    ap.add_argument("--channels", type=int, default=3, choices=(3, 4), help="channels of the developed image")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch

    import amvpt.display as D

    assert torch.cuda.is_available(), "display_bench.py needs a GPU"
    qw, qh = a.quilt
    dw, dh = a.size
    gen = torch.Generator(device="cuda").manual_seed(1)
    image = torch.rand((qh, qw, a.channels), dtype=torch.float32, device="cuda", generator=gen) * 1.1 - 0.05
    quilt = torch.zeros(qh * qw * 3 + 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(dh * dw * 3 + 4, dtype=torch.uint8, device="cuda")
    preset = D.default_preset()

    def srgb(off):
        D.srgb8_device(image.data_ptr(), a.channels, qw, qh, quilt.data_ptr() + off)

    def lace(off):
        D.interlace_device(quilt.data_ptr(), qw, qh, 3, out.data_ptr() + off, (dw, dh), preset)

    variants = {"k_srgb8": (srgb, 0), "k_srgb8_scalar_bytes": (srgb, 1),
                "k_interlace": (lace, 0), "k_interlace_byte_stores": (lace, 1)}
    times = {k: [] for k in variants}
    for fn, off in variants.values():
        for _ in range(a.warmup):
            fn(off)
    torch.cuda.synchronize()
    for _ in range(a.repeats):          # the variants alternate inside every repeat
        for name, (fn, off) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(off)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    srgb_bytes = qw * qh * (a.channels * 4 + 3)
    lace_bytes = qw * qh * 3 + dw * dh * 3
    res = {"quilt": [qw, qh], "size": [dw, dh], "image_channels": a.channels, "repeats": a.repeats,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_per_s": HBM_PEAK_GBS}
    for name in variants:
        res[name] = stats(times[name], srgb_bytes if name.startswith("k_srgb8") else lace_bytes)
    res["stage_median_ms"] = round(res["k_srgb8"]["median_ms"] + res["k_interlace"]["median_ms"], 4)
    # the dword-store image and the byte-store image are the same bytes
    lace(0)
    ref = out[:dh * dw * 3].clone()
    lace(1)
    res["byte_store_image_equal"] = bool(torch.equal(ref, out[1:dh * dw * 3 + 1]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Splat time per reconstruction filter, row-reduced splat against the block window.

At config M's shape (8 views of 1024^2 on a 4 x 2 grid, 64 spp as 4 passes of 16, G = 8) renders one frame per
variant -- the default Gaussian, tent, Mitchell-Netravali and Catmull-Rom, each plain (the row splat where the
filter has one) and with AMVPT_OPT_BLOCK_SPLAT (the per-lane block window of the same build) -- and reads the
splat's HIP-event time from amvpt_counters.kernel_ms[AMVPT_K_SPLAT].  The variants are interleaved (every round
runs all of them once), so drift hits all alike; the spread is the range over the rounds of the same variant.

    python tools/rfilter_splat.py [--rounds 5] [--res 1024] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "mitsuba3-amvpt_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FILTERS = ["gaussian", "tent", "mitchell", "catmullrom"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch

    import amvpt

    assert torch.cuda.is_available(), "needs a GPU"
    scene_file = os.path.join(REPO, "scenes", "cbox_grid.xml")
    variants = []
    for name in FILTERS:
        s = amvpt.load_file(scene_file, res=args.res, spp=args.spp, gx=4, gy=2, reuse=8, rfilter=name)
        sd, vd, p = s.describe(0, 0, 0)
        dev = amvpt.DeviceScene(sd)
        for block in (False, True):
            variants.append(dict(name=name, block=block, scene=s, dev=dev, vd=vd, p=p, ms=[], total=[]))
    p = variants[0]["p"]
    film = torch.zeros((p.film_height, p.film_width, 4), dtype=torch.float32, device="cuda")

    def frame(v):
        film.zero_()
        cnt = amvpt.Counters()
        v["dev"].render_ex(v["vd"], v["p"], film.data_ptr(), flags=amvpt.OPT_BLOCK_SPLAT if v["block"] else 0,
                           counters=cnt)
        torch.cuda.synchronize()
        return cnt.kernel_ms[amvpt.KERNELS.index("k_splat")], cnt.total_ms

    for v in variants:   # warm-up: arena allocation, code upload
        frame(v)
    for _ in range(args.rounds):
        for v in variants:
            ms, total = frame(v)
            v["ms"].append(ms)
            v["total"].append(total)

    rows = []
    print("%-11s %-6s %10s %10s %10s %10s" % ("filter", "splat", "median ms", "min", "max", "frame ms"))
    for v in variants:
        row = dict(filter=v["name"], path="block" if v["block"] else "plain", splat_ms_median=statistics.median(v["ms"]),
                   splat_ms_min=min(v["ms"]), splat_ms_max=max(v["ms"]), frame_ms_median=statistics.median(v["total"]),
                   splat_ms=v["ms"])
        rows.append(row)
        print("%-11s %-6s %10.2f %10.2f %10.2f %10.2f" % (row["filter"], row["path"], row["splat_ms_median"],
                                                          row["splat_ms_min"], row["splat_ms_max"],
                                                          row["frame_ms_median"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(res=args.res, spp=args.spp, rounds=args.rounds, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()

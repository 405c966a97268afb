#!/usr/bin/env python3
"""Times a frame into the float film and into the fixed-point film (include/amvpt_fixed.h) on one GPU.

Shapes: bench.py's config M and its mesh config.  Each frame is rendered these ways, alternating inside every repeat:

    float        render_ex, the float film (the row-reduced splat where it is eligible)
    fixed        render_fixed, the integer LDS-window splat
    fixed_direct render_fixed | OPT_FIXED_DIRECT: one global integer atomic per footprint cell
    flag         render_ex | OPT_DETERMINISTIC: a private fixed-point film, cleared and resolved in the call

A library without amvpt_render_fixed (AMVPT_LIB_DIR pointing at an older build) gets `float` and `flag` only: its
flag path is its direct put.  Reported per way: whole-frame milliseconds (HIP events around the call, the film's
clear and the one resolve included for the fixed ways, as a caller pays them) and the AMVPT_K_SPLAT kernel time of
amvpt_counters, as median, min and max over the repeats after the warm-up frames.  Every frame is an instrumented
render (counters: per-kernel events and a host synchronisation), so the frame times are comparable with each other,
not with bench.py's.  Prints one JSON object.

    python tools/fixed_film_bench.py [--configs M mesh] [--repeats 5] [--warmup 1] [--res N] [--spp N] [--no-direct]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mitsuba3-amvpt_amd"))

CONFIGS = {   # bench.py's
    "M": dict(scene="cbox_grid.xml", res=1024, spp=64, gx=4, gy=2, reuse=8, adaptive=0),
    "mesh": dict(scene="cbox_mesh.xml", res=1024, spp=64, gx=4, gy=2, reuse=8, adaptive=0),
}


def spread(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["M", "mesh"], choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--res", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--no-direct", action="store_true", help="leave fixed_direct out (12 s a frame at config M)")
    a = ap.parse_args()

    import torch

    import amvpt

    assert torch.cuda.is_available(), "fixed_film_bench.py needs a GPU"
    has_fixed = hasattr(amvpt.hip_lib(), "amvpt_render_fixed")
    det = amvpt.OPT_DETERMINISTIC
    direct = getattr(amvpt, "OPT_FIXED_DIRECT", 1024)
    res = {"device": torch.cuda.get_device_name(0), "lib_dir": os.path.relpath(amvpt.LIB_DIR, REPO),
           "render_fixed": has_fixed, "repeats": a.repeats, "warmup": a.warmup, "configs": {}}
    for name in a.configs:
        cfg = dict(CONFIGS[name])
        if a.res:
            cfg["res"] = a.res
        if a.spp:
            cfg["spp"] = a.spp
        scene = amvpt.load_file(os.path.join(REPO, "scenes", cfg.pop("scene")), **cfg)
        sd, vd, p = scene.describe(0, 0, 0)
        dev = amvpt.DeviceScene(sd)
        shape = (p.film_height, p.film_width, 5 if p.film_alpha else 4)
        film = torch.zeros(shape, dtype=torch.float32, device="cuda")
        fixed = torch.zeros(shape, dtype=torch.int64, device="cuda")

        def float_way(flags):
            def run(cnt):
                film.zero_()
                dev.render_ex(vd, p, film.data_ptr(), flags=flags, counters=cnt)
            return run

        def fixed_way(flags):
            def run(cnt):
                fixed.zero_()
                dev.render_fixed(vd, p, fixed.data_ptr(), flags=flags, counters=cnt)
                amvpt.fixed_resolve(fixed.data_ptr(), film.data_ptr(), fixed.numel())
            return run

        ways = {"float": float_way(0), "flag": float_way(det)}
        if has_fixed:
            ways["fixed"] = fixed_way(0)
            if not a.no_direct:
                ways["fixed_direct"] = fixed_way(direct)
        frame_ms = {k: [] for k in ways}
        splat_ms = {k: [] for k in ways}
        for it in range(a.warmup + a.repeats):
            for k, run in ways.items():
                cnt = amvpt.Counters()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(cnt)
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    frame_ms[k].append(e0.elapsed_time(e1))
                    splat_ms[k].append(cnt.kernel_ms_splat)
        out = {"film": list(shape), "lanes_per_frame": int(cnt.lanes), "ways": {}}
        for k in ways:
            out["ways"][k] = {"frame_ms": spread(frame_ms[k]), "k_splat_ms": spread(splat_ms[k])}
        if has_fixed:
            out["fixed_over_float_frame"] = round(out["ways"]["fixed"]["frame_ms"]["median"] /
                                                  out["ways"]["float"]["frame_ms"]["median"], 4)
        if "fixed_direct" in ways:
            out["fixed_over_direct_k_splat"] = round(out["ways"]["fixed"]["k_splat_ms"]["median"] /
                                                     out["ways"]["fixed_direct"]["k_splat_ms"]["median"], 4)
        res["configs"][name] = out
        del dev, film, fixed
    print(json.dumps(res))


if __name__ == "__main__":
    main()

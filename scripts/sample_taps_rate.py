#!/usr/bin/env python3
"""Frame time of the sample-table calls (c2rt_render_frame_taps_device, c2rt_render_frame_adaptive_taps_device) next to what
they replace or compete with, everything resident in HBM, on lecture5.sdl and lecture4.sdl at 1920x1080 and 3840x2160:

  (a1) taps grid16          the whole frame at tap_grid(4), ONE launch
  (a2) compose grid16       what a caller did before: per tap, torch builds the W * H rays on the device (48 B per ray),
                            c2rt_trace_rays_device with rgb only (12 B per sample), torch adds; one division at the end
  (b1) taps ref5            the reference's five taps through the new call
  (b2) frame 5 taps         c2rt_render_frame_device with C2RT_TAPS_REF5: the same bits from the frame kernel
  (c1) adaptive grid16      c2rt_render_frame_adaptive_taps_device: 15 taps on the flagged pixels only
  (c2) adaptive ref5        c2rt_render_frame_adaptive_device: 4 taps on the flagged pixels

The composition's frame is compared with (a1)'s once, outside the timed windows, and the number of floats that differ is
printed (torch restates the screen ray in fp64 tensor operations, one kernel each; it is a timing arm, not a yardstick).

Every shape is warmed up; every timed window holds at least --window-ms of work (default 500) behind a settling phase and
is timed with device events on the stream; the legs are interleaved --rounds times in one process and the median,
minimum and maximum are printed.

  python scripts/sample_taps_rate.py [--rounds 5] [--json out.json]
  python scripts/sample_taps_rate.py --adaptive-only   (c1) and (c2) alone; the library variant is the one C2RT_LIB_VARIANT names
  python scripts/sample_taps_rate.py --once      one pass of (a1), (a2), (c1) per case and nothing else (under rocprofv3
                                                 --kernel-trace --stats: the 16 trace kernels' sum, the refinement kernel)
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import chess2rt_amd as c2
from chess2rt_amd import _abi

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
CASES = [("lecture5.sdl", 1920, 1080), ("lecture5.sdl", 3840, 2160), ("lecture4.sdl", 1920, 1080), ("lecture4.sdl", 3840, 2160)]


def vec(cam, name, dev):
    return torch.tensor(list(getattr(cam, name)), dtype=torch.float64, device=dev)


def build_rays(cam, xs, ys, dx, dy, rays):
    """Camera.getScreenRay and raytrace()'s normalisation for the screen points (xs + dx, ys + dy) into rays (n, 6)"""
    dev = xs.device
    pos, ul = vec(cam, "pos", dev), vec(cam, "up_left", dev)
    ur, dl = vec(cam, "up_right", dev), vec(cam, "down_left", dev)
    fx, fy = (xs + dx) / cam.frame_width, (ys + dy) / cam.frame_height
    raw = (ul + (ur - ul) * fx[:, None]) + (dl - ul) * fy[:, None] - pos
    inv = 1.0 / torch.sqrt((raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]) + raw[:, 2] * raw[:, 2])
    rays[:, :3] = pos
    rays[:, 3:] = raw * inv[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=500.0)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--adaptive-only", action="store_true", help="only the two adaptive legs (variant builds of the refinement kernel)")
    ap.add_argument("--json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = c2.Context(0)
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream
    grid16, ref5 = c2.tap_grid(4), c2.TAPS_REF5_TABLE
    rows = []
    for scene_file, w, h in CASES:
        n = w * h
        scene = c2.parseSceneFromFile(os.path.join(SCENES, scene_file))
        scene.setFrameSize(w, h)
        scene.setAA(True)
        scene.setDof(False)
        cam = scene.beginFrame()
        five, one = scene.renderOpts(taps=_abi.TAPS_REF5), scene.renderOpts(taps=_abi.TAPS_1)
        ctx.uploadScene(scene.desc)
        frame_t = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        mask_t = torch.empty((h, w), dtype=torch.uint8, device=dev)
        rays_t = torch.empty((n, 6), dtype=torch.float64, device=dev)
        rgb_t = torch.empty((n, 3), dtype=torch.float32, device=dev)
        sum_t = torch.empty((n, 3), dtype=torch.float32, device=dev)
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing="ij")
        xs, ys = xs.reshape(-1), ys.reshape(-1)

        def compose():
            with torch.cuda.stream(st):
                for t, (dx, dy) in enumerate(grid16):
                    build_rays(cam, xs, ys, dx, dy, rays_t)
                    ctx.traceRaysDevice(rays_t.data_ptr(), n, 0, rgb_t.data_ptr(), s)
                    if t == 0:
                        sum_t.copy_(rgb_t)
                    else:
                        sum_t.add_(rgb_t)
                sum_t.div_(float(len(grid16)))

        legs = {
            "(a1) taps grid16": lambda: ctx.renderFrameTapsDevice(cam, one, grid16, frame_t.data_ptr(), stream=s),
            "(a2) compose grid16": compose,
            "(b1) taps ref5": lambda: ctx.renderFrameTapsDevice(cam, one, ref5, frame_t.data_ptr(), stream=s),
            "(b2) frame 5 taps": lambda: ctx.renderFrameDevice(cam, five, frame_t.data_ptr(), s),
            "(c1) adaptive grid16": lambda: ctx.renderFrameAdaptiveTapsDevice(cam, one, grid16, frame_t.data_ptr(), mask_t.data_ptr(), stream=s),
            "(c2) adaptive ref5": lambda: ctx.renderFrameAdaptiveDevice(cam, five, frame_t.data_ptr(), mask_t.data_ptr(), stream=s),
        }
        name = "%s %dx%d" % (scene_file, w, h)
        # once, untimed: the flagged share, and the composition against the call
        legs["(c1) adaptive grid16"]()
        torch.cuda.synchronize()
        share = float(mask_t.to(torch.float32).mean().item())
        legs["(a2) compose grid16"]()
        legs["(a1) taps grid16"]()
        torch.cuda.synchronize()
        differ = int((sum_t.view(torch.int32) != frame_t.view(n, 3).view(torch.int32)).sum())
        print("%-24s flagged share %.4f; composition against the call: %d of %d floats differ" % (name, share, differ, n * 3), flush=True)
        if args.once:
            continue
        if args.adaptive_only:
            legs = {k: v for k, v in legs.items() if k.startswith("(c")}
        passes = {}
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def window(leg, count):
            start.record(st)
            for _ in range(count):
                leg()
            stop.record(st)
            stop.synchronize()
            return start.elapsed_time(stop) * 1e-3 / count

        for k, leg in legs.items():
            leg()
            torch.cuda.synchronize()
            passes[k] = max(3, int(math.ceil(args.window_ms * 1e-3 / window(leg, 3))))
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                for _ in range(max(2, passes[k] // 8)):   # settling phase
                    leg()
                torch.cuda.synchronize()
                times[k].append(window(leg, passes[k]))
        for k in legs:
            med = statistics.median(times[k])
            rows.append({"case": name, "leg": k, "pixels": n, "flagged_share": round(share, 5), "us_median": round(med * 1e6, 2),
                         "us_min": round(min(times[k]) * 1e6, 2), "us_max": round(max(times[k]) * 1e6, 2),
                         "windows_us": [round(x * 1e6, 2) for x in times[k]], "passes_per_window": passes[k]})
            print("%-24s %-22s %10.1f us [%.1f..%.1f]  (%d passes/window)" % (name, k, med * 1e6, min(times[k]) * 1e6, max(times[k]) * 1e6, passes[k]), flush=True)
        r = {row["leg"][:4]: row for row in rows if row["case"] == name}
        if not args.adaptive_only:
            print("%-24s (a) compose / taps = %.2f (windows apart: %s);  (b) taps ref5 / frame = %.2f;  (c) adaptive16 / whole16 = %.3f, adaptive16 / adaptive5 = %.2f"
                  % (name, r["(a2)"]["us_median"] / r["(a1)"]["us_median"], r["(a1)"]["us_max"] < r["(a2)"]["us_min"],
                     r["(b1)"]["us_median"] / r["(b2)"]["us_median"], r["(c1)"]["us_median"] / r["(a1)"]["us_median"],
                     r["(c1)"]["us_median"] / r["(c2)"]["us_median"]), flush=True)
        del rays_t, rgb_t, sum_t, frame_t, mask_t, xs, ys
        torch.cuda.empty_cache()
    if args.json and rows:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Frame time of adaptive anti-aliasing (c2rt_render_frame_adaptive_device) next to the five-tap and the one-tap frame
of the same camera, everything resident in HBM:

  lecture5.sdl 3840x2160 and 1920x1080   the headline scene: flags along edges only
  lecture4.sdl 1920x1080                 the adverse case: the far checker rows flag densely

Legs per case: the C2RT_TAPS_REF5 frame, the C2RT_TAPS_1 frame, the adaptive call; the flagged share of the mask is
printed with them.  Every timed window holds at least --window-ms of work behind a settling phase and ends in a device
sync; the legs are interleaved --rounds times and the median, minimum and maximum are printed.  The library variant under
test is the one C2RT_LIB_VARIANT names (the plain refinement kernel the packed one was measured against,
profiles/adaptive_aa.md, is no longer built).

  python scripts/adaptive_aa_rate.py [--rounds 5] [--json out.json]
  python scripts/adaptive_aa_rate.py --once          one adaptive call per case and nothing else (under rocprofv3
                                                     --kernel-trace --stats: the detect and refine kernel times)
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import chess2rt_amd as c2
from chess2rt_amd import _abi

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
CASES = [("lecture5.sdl", 3840, 2160), ("lecture5.sdl", 1920, 1080), ("lecture4.sdl", 1920, 1080)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--adaptive-only", action="store_true", help="skip the plain frame legs (variant builds)")
    ap.add_argument("--json")
    args = ap.parse_args()
    variant = os.environ.get("C2RT_LIB_VARIANT", "") or "default"
    dev = torch.device("cuda:0")
    ctx = c2.Context(0)
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream
    rows = []
    for scene_file, w, h in CASES:
        scene = c2.parseSceneFromFile(os.path.join(SCENES, scene_file))
        scene.setFrameSize(w, h)
        scene.setAA(True)
        scene.setDof(False)
        cam = scene.beginFrame()
        five, one = scene.renderOpts(taps=_abi.TAPS_REF5), scene.renderOpts(taps=_abi.TAPS_1)
        ctx.uploadScene(scene.desc)
        frame_t = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        mask_t = torch.empty((h, w), dtype=torch.uint8, device=dev)
        adaptive = lambda: ctx.renderFrameAdaptiveDevice(cam, five, frame_t.data_ptr(), mask_t.data_ptr(), stream=s)
        adaptive()
        torch.cuda.synchronize()
        share = float(mask_t.to(torch.float32).mean().item())
        name = "%s %dx%d" % (scene_file, w, h)
        print("%-10s %-26s flagged share %.4f" % (variant, name, share), flush=True)
        if args.once:
            continue
        legs = {}
        if not args.adaptive_only:
            legs["frame 5 taps"] = lambda: ctx.renderFrameDevice(cam, five, frame_t.data_ptr(), s)
            legs["frame 1 tap"] = lambda: ctx.renderFrameDevice(cam, one, frame_t.data_ptr(), s)
        legs["adaptive"] = adaptive
        passes = {}
        for k, leg in legs.items():
            leg()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(3):
                leg()
            torch.cuda.synchronize()
            passes[k] = max(3, int(math.ceil(args.window_ms * 1e-3 / ((time.perf_counter() - t) / 3) * 1.25)))
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                for _ in range(max(2, passes[k] // 4)):   # settling phase
                    leg()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(passes[k]):
                    leg()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t) / passes[k])
        for k in legs:
            med = statistics.median(times[k])
            rows.append({"variant": variant, "case": name, "leg": k, "flagged_share": round(share, 5), "us_median": round(med * 1e6, 2),
                         "us_min": round(min(times[k]) * 1e6, 2), "us_max": round(max(times[k]) * 1e6, 2), "passes_per_window": passes[k]})
            print("%-10s %-26s %-14s %9.1f us [%.1f..%.1f]  (%d passes/window)" % (variant, name, k, med * 1e6, min(times[k]) * 1e6, max(times[k]) * 1e6, passes[k]), flush=True)
    if args.json and rows:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

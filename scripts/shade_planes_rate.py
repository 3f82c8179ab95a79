#!/usr/bin/env python3
"""Time per frame of the shading planes (c2rt_render_shading_device) on lecture5.sdl at 1920x1080, everything resident
in HBM, next to the hit planes and to what a caller did for the same information before the call existed:

  (a) hits rgb             c2rt_render_hits_device, rgb only: the hit planes' kernel, the reference point
  (b) shading rgb          c2rt_render_shading_device, rgb only: same trace, same shading, same store
  (c) shading all six      node, albedo, light, specular, visible, rgb
  (d) shading node+albedo  no shadow ray, no light
  (e) hits + visibility    c2rt_render_hits_device with node, uv, p, normal, rgb, then c2rt_test_visibility_device over
                           hits x lights segments (built once, outside the timed loop: the pass that builds them, and the
                           texture and light arithmetic on the host, which a real caller also pays, are not counted)

Every timed window holds at least --window-ms of work behind a settling phase and ends in a device sync; the arms are
interleaved --rounds times in one process and the median, minimum and maximum are printed.

  python scripts/shade_planes_rate.py [--rounds 7] [--json out.json]
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
import numpy as np
import torch

import chess2rt_amd as c2
from chess2rt_amd.api import HIT_PLANES, SHADE_PLANES

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def device_planes(table, n, dev):
    return {k: torch.empty(n * comps, dtype=torch.from_numpy(np.empty(0, dtype=t)).dtype, device=dev) for k, (t, comps) in table.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--json")
    args = ap.parse_args()
    w, h = args.size
    n = w * h
    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    scene.setFrameSize(w, h)
    scene.setAA(False)
    scene.setDof(False)
    cam = scene.beginFrame()
    opts = scene.renderOpts(taps=1)
    ctx = c2.Context(0)
    ctx.uploadScene(scene.desc)
    dev = torch.device("cuda:0")
    hit_t = device_planes(HIT_PLANES, n, dev)
    hit_ptrs = {k: v.data_ptr() for k, v in hit_t.items()}
    shade_t = device_planes(SHADE_PLANES, n, dev)
    shade_ptrs = {k: v.data_ptr() for k, v in shade_t.items()}
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream

    # the segments of arm (e): p + N * 1e-6 -> every light, for every hit, N the normal turned against the ray
    d = scene.desc.contents
    lights = np.array([d.light_pos[i] for i in range(3 * d.n_lights)], dtype=np.float64).reshape(-1, 3)
    pl = ctx.renderHits(cam, opts, planes=("node", "p", "normal"))
    hit = pl["node"].reshape(-1) >= 0
    p, nrm = pl["p"].reshape(-1, 3)[hit], pl["normal"].reshape(-1, 3)[hit]
    rd = p - np.array(list(cam.pos))
    N = np.where(((rd * nrm).sum(axis=1) < 0)[:, None], nrm, -nrm)
    seg = np.empty((len(p), len(lights), 6), dtype=np.float64)
    seg[:, :, :3] = (p + N * 1e-6)[:, None, :]
    seg[:, :, 3:] = lights[None, :, :]
    n_seg = len(p) * len(lights)
    seg_t = torch.from_numpy(np.ascontiguousarray(seg.reshape(n_seg, 6))).to(dev)
    vis_t = torch.empty(max(n_seg, 1), dtype=torch.uint8, device=dev)
    today = {k: hit_ptrs[k] for k in ("node", "uv", "p", "normal", "rgb")}

    def arm_e():
        ctx.renderHitsDevice(cam, opts, today, s)
        ctx.testVisibilityDevice(seg_t.data_ptr(), n_seg, vis_t.data_ptr(), s)

    legs = {}
    legs["(a) hits rgb"] = lambda: ctx.renderHitsDevice(cam, opts, {"rgb": hit_ptrs["rgb"]}, s)
    legs["(b) shading rgb"] = lambda: ctx.renderShadingDevice(cam, opts, {"rgb": shade_ptrs["rgb"]}, s)
    legs["(c) shading all six"] = lambda: ctx.renderShadingDevice(cam, opts, shade_ptrs, s)
    legs["(d) shading node+albedo"] = lambda: ctx.renderShadingDevice(cam, opts, {"node": shade_ptrs["node"], "albedo": shade_ptrs["albedo"]}, s)
    legs["(e) hits + visibility"] = arm_e
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
    rows = []
    for k in legs:
        med = statistics.median(times[k])
        rows.append({"leg": k, "pixels": n, "segments": n_seg if k.startswith("(e)") else 0, "us_median": round(med * 1e6, 2),
                     "us_min": round(min(times[k]) * 1e6, 2), "us_max": round(max(times[k]) * 1e6, 2), "passes_per_window": passes[k]})
        print("%-26s %9.1f us [%.1f..%.1f]  (%d passes/window)" % (k, med * 1e6, min(times[k]) * 1e6, max(times[k]) * 1e6, passes[k]), flush=True)
    med = {r["leg"][:3]: r["us_median"] for r in rows}
    print("(c) / (e) = %.3f   (b) - (a) = %+.1f us   (c) - (b) = %+.1f us   %d of %d pixels hit, %d lights" %
          (med["(c)"] / med["(e)"], med["(b)"] - med["(a)"], med["(c)"] - med["(b)"], int(hit.sum()), n, len(lights)), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

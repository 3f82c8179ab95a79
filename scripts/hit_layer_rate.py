#!/usr/bin/env python3
"""Cost of the hit layers (c2rt_trace_rays_layers_device, c2rt_render_hit_layers_device) on lecture5.sdl's 1920x1080
screen rays, everything resident in HBM:

  (a) the ray face at max_layers 1, 2, 4 and 8 — hits + colour, hits only, count only
  (b) c2rt_trace_rays_device on the same rays, three times over (the spread of its repeated medians is the yardstick
      for "max_layers = 1 costs the same")
  (c) the route a caller had before: max_layers calls of c2rt_trace_rays_device, with the stepping, the masking of the
      rays that missed and the scatter into layer-major arrays done by torch on the device in between — after a check
      that it gives the same bits
  (d) the frame face (all seven planes + count) at 1, 4 and 8 layers against c2rt_render_hits_device

Every timed window holds at least --window-ms of work behind a settling phase and ends in a device sync; the legs are
interleaved --rounds times and the median, minimum and maximum are printed, then the distribution of `count` and the
share of the 8-layer time that the layers behind the second take.

  python scripts/hit_layer_rate.py [--rounds 5] [--json out.json]
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
from chess2rt_amd.api import HIT_PLANES

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
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
    # Camera.getScreenRay (rt/camera.d:123-154), vectorised: the exact bits do not matter to a rate
    ul, ur, dl, pos = (np.array(list(v)) for v in (cam.up_left, cam.up_right, cam.down_left, cam.pos))
    xs, ys = np.meshgrid(np.arange(w) / cam.frame_width, np.arange(h) / cam.frame_height)
    d = ul + (ur - ul) * xs[..., None] + (dl - ul) * ys[..., None] - pos
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(n, 3)
    rays = np.ascontiguousarray(np.hstack([np.broadcast_to(pos, d.shape), d]))
    dev = torch.device("cuda:0")
    KMAX = 8
    rays_t = torch.from_numpy(rays).to(dev)
    hits_t = torch.zeros((KMAX, n, 10), dtype=torch.float64, device=dev)        # c2rt_ray_hit as ten 8-byte words
    rgb_t = torch.zeros((KMAX, n, 3), dtype=torch.float32, device=dev)
    count_t = torch.zeros(n, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream

    # ---- (c) the route through the single-hit call, torch in between ----------------------------------------------------
    one_hits = torch.zeros((n, 10), dtype=torch.float64, device=dev)
    one_rgb = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    ref_hits, ref_rgb, ref_count = torch.zeros_like(hits_t), torch.zeros_like(rgb_t), torch.zeros_like(count_t)

    def torch_route(K, out_hits, out_rgb, out_count):
        with torch.cuda.stream(st):
            cur, idx = rays_t, torch.arange(n, device=dev)
            total = torch.zeros(n, dtype=torch.float64, device=dev)
            out_count.zero_()
            for k in range(K):
                m = cur.shape[0]
                if m == 0:
                    break
                ctx.traceRaysDevice(cur.data_ptr(), m, one_hits.data_ptr(), one_rgb.data_ptr(), s)
                rec = one_hits[:m].clone()
                hit = rec[:, 0].contiguous().view(torch.int32).view(m, 2)[:, 0] >= 0      # closest_node: the low word
                rec[:, 1] = torch.where(hit, rec[:, 1] + total[idx], rec[:, 1])
                out_hits[k, idx] = rec
                out_rgb[k, idx] = one_rgb[:m]
                idx_hit = idx[hit]                               # the host waits here: the next launch needs its size
                total[idx_hit] = rec[hit, 1]
                out_count[idx_hit] += 1
                step = cur[hit, 3:] * 1e-6
                cur = torch.cat([rec[hit, 4:7] + step, cur[hit, 3:]], dim=1).contiguous()
                idx = idx_hit

    def layers(K, hits=True, rgb=True, count=True):
        ctx.traceRayLayersDevice(rays_t.data_ptr(), n, K, hits_t.data_ptr() if hits else 0, rgb_t.data_ptr() if rgb else 0,
                                 count_t.data_ptr() if count else 0, s)

    # the check: the route's bits are the call's, on every slot the rule writes
    torch.cuda.synchronize()
    layers(KMAX)
    torch_route(KMAX, ref_hits, ref_rgb, ref_count)
    torch.cuda.synchronize()
    count = count_t.cpu().numpy()
    assert np.array_equal(count, ref_count.cpu().numpy()), "count differs between the call and the torch route"
    written = torch.from_numpy(np.arange(KMAX)[:, None] <= count[None, :].astype(np.int64)).to(dev)
    assert torch.equal(hits_t.view(torch.int64)[written], ref_hits.view(torch.int64)[written]), "records differ"
    assert torch.equal(rgb_t.view(torch.int32)[written], ref_rgb.view(torch.int32)[written]), "colours differ"
    hist = np.bincount(count, minlength=KMAX + 1)
    print("count histogram over %d rays: %s" % (n, hist.tolist()), flush=True)

    # ---- the legs ----------------------------------------------------------------------------------------------------------
    legs = {}
    for K in (1, 2, 4, 8):
        legs["(a) layers K=%d hits+colour+count" % K] = lambda K=K: layers(K)
        legs["(a) layers K=%d hits+count" % K] = lambda K=K: layers(K, rgb=False)
        legs["(a) layers K=%d count only" % K] = lambda K=K: layers(K, hits=False, rgb=False)
    for rep in (1, 2, 3):
        legs["(b) trace_rays hits+colour #%d" % rep] = lambda: ctx.traceRaysDevice(rays_t.data_ptr(), n, one_hits.data_ptr(), one_rgb.data_ptr(), s)
    for K in (4, 8):
        legs["(c) torch route K=%d" % K] = lambda K=K: torch_route(K, ref_hits, ref_rgb, ref_count)
    planes = {}
    for name, (dtype, comps) in HIT_PLANES.items():
        planes[name] = torch.zeros(KMAX * n * comps * np.dtype(dtype).itemsize, dtype=torch.uint8, device=dev)
    ptrs = {k: v.data_ptr() for k, v in planes.items()}
    legs["(d) render_hits all planes"] = lambda: ctx.renderHitsDevice(cam, opts, ptrs, s)
    for K in (1, 4, 8):
        legs["(d) hit layers K=%d all planes+count" % K] = lambda K=K: ctx.renderHitLayersDevice(cam, opts, K, ptrs, count_t.data_ptr(), s)

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
    rows, med = [], {}
    for k in legs:
        med[k] = statistics.median(times[k])
        rows.append({"leg": k, "rays": n, "us_median": round(med[k] * 1e6, 2), "us_min": round(min(times[k]) * 1e6, 2),
                     "us_max": round(max(times[k]) * 1e6, 2), "passes_per_window": passes[k]})
        print("%-40s %9.1f us [%.1f..%.1f]  (%d passes/window)" % (k, med[k] * 1e6, min(times[k]) * 1e6, max(times[k]) * 1e6, passes[k]), flush=True)
    b = [med["(b) trace_rays hits+colour #%d" % r] for r in (1, 2, 3)]
    a1 = med["(a) layers K=1 hits+colour+count"]
    print("K=1 against (b): %.1f us against %.1f us (medians of (b): %.1f .. %.1f, spread %.1f us)" %
          (a1 * 1e6, statistics.median(b) * 1e6, min(b) * 1e6, max(b) * 1e6, (max(b) - min(b)) * 1e6))
    for K in (4, 8):
        print("K=%d against the torch route: %.1f us against %.1f us, ratio %.2f" %
              (K, med["(a) layers K=%d hits+colour+count" % K] * 1e6, med["(c) torch route K=%d" % K] * 1e6,
               med["(c) torch route K=%d" % K] / med["(a) layers K=%d hits+colour+count" % K]))
    t2, t8 = med["(a) layers K=2 hits+colour+count"], med["(a) layers K=8 hits+colour+count"]
    print("share of the K=8 time behind the second layer: %.1f %% (%.1f of %.1f us)" % ((t8 - t2) / t8 * 100, (t8 - t2) * 1e6, t8 * 1e6))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"count_histogram": hist.tolist(), "legs": rows}, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

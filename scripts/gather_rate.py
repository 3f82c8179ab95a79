#!/usr/bin/env python3
"""Time per frame of the gather planes (c2rt_render_gather_device) on lecture5.sdl at 1920x1080, everything resident in
HBM, next to the route a caller had for the same `bounce` plane before the call existed, each part of that timed on its
own:

  (a)  gather bounce, K = 16     c2rt_render_gather_device, `bounce` only
  (b)  gather all four           node, hits, indirect, bounce
  (c1) hit planes                c2rt_render_hits_device with node, p, normal
  (c2) shading planes            c2rt_render_shading_device with albedo
  (c3) torch: rays               the K rays of every hit and their weights, built on the device from the same counter
                                 RNG (48 B x K per hit written), sample-major
  (c4) trace_rays x K            K launches of c2rt_trace_rays_device with colours, one per sample index
  (c5) torch: sums               the K weighted fp32 sums, the division and the product with the albedo
  (d1)  gather bounce, K = 1     the cost per sample: (a) at one sample
  (d64) gather bounce, K = 64    and at 64
  (e1) / (e64) gather all four at K = 1 / 64

The composition's `bounce` is compared with (b)'s once, outside the timed loops, and the number of pixels that differ
is printed (torch evaluates the definition's operations one kernel each, so nothing is contracted).

Every timed window holds at least --window-ms of work behind a settling phase and ends in a device sync; the legs are
interleaved --rounds times in one process and the median, minimum and maximum are printed.  The expectation held
against the numbers: (a) <= (c1) + (c2) + (c4), the kernels of the composed route alone, the allowance being the spread
of the windows of those legs.

  python scripts/gather_rate.py [--rounds 5] [--json out.json]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch

import chess2rt_amd as c2
from chess2rt_amd.api import GATHER_PLANES, HIT_PLANES, SHADE_PLANES
from occlusion_rate import SCENES, device_planes, rng_key, rng_uniform, sincos2pi   # the definition's sample generator in torch


def build_rays(node, p, normal, d, K, seed, rays_out, w_out):
    """the K rays of every hit into rays_out[k][: hits] (sample-major) and their weights into w_out[k][: hits]; returns
    (indices of the hits, their count)"""
    idx = torch.nonzero(node >= 0).reshape(-1)
    nrm, rd = normal[idx], d[idx]
    front = ((rd[:, 0] * nrm[:, 0] + rd[:, 1] * nrm[:, 1]) + rd[:, 2] * nrm[:, 2]) < 0
    N = torch.where(front[:, None], nrm, -nrm)
    frm = p[idx] + N * 1e-6
    key = rng_key(seed, idx)[None, :]
    s = torch.arange(K, device=node.device, dtype=torch.int64)[:, None]
    u, v = rng_uniform(key, s, 0), rng_uniform(key, s, 1)
    sn, cs = sincos2pi(u)
    w = 2.0 * v - 1.0
    c = torch.sqrt(1.0 - w * w)
    res = torch.stack([cs * c, -w, sn * c], dim=-1)                                     # [K][hits][3]
    flip = ((res[..., 0] * N[None, :, 0] + res[..., 1] * N[None, :, 1]) + res[..., 2] * N[None, :, 2]) < 0
    res = torch.where(flip[..., None], -res, res)
    m = len(idx)
    rays = rays_out[: K * m * 6].view(K, m, 6)
    rays[:, :, :3] = frm[None, :, :]
    rays[:, :, 3:] = res
    cosw = (res[..., 0] * N[None, :, 0] + res[..., 1] * N[None, :, 1]) + res[..., 2] * N[None, :, 2]
    w_out[: K * m].view(K, m)[:] = (2.0 * cosw).to(torch.float32)
    return idx, m


def reduce_colours(rgb, wts, albedo, idx, m, K, n, bounce_out):
    L, w = rgb[: K * m * 3].view(K, m, 3), wts[: K * m].view(K, m)
    total = torch.zeros(m, 3, dtype=torch.float32, device=rgb.device)
    for s in range(K):
        total = total + L[s] * w[s][:, None]
    bounce_out.zero_()
    bounce_out.view(n, 3)[idx] = albedo.view(n, 3)[idx] * (total / float(K))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--json")
    args = ap.parse_args()
    w, h = args.size
    n, K = w * h, args.samples
    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    scene.setFrameSize(w, h)
    scene.setAA(False)
    scene.setDof(False)
    cam = scene.beginFrame()
    opts = scene.renderOpts(taps=1)
    ctx = c2.Context(0)
    ctx.uploadScene(scene.desc)
    dev = torch.device("cuda:0")
    hit_t = device_planes({k: HIT_PLANES[k] for k in ("node", "p", "normal")}, n, dev)
    hit_ptrs = {k: v.data_ptr() for k, v in hit_t.items()}
    alb_t = device_planes({"albedo": SHADE_PLANES["albedo"]}, n, dev)
    alb_ptrs = {"albedo": alb_t["albedo"].data_ptr()}
    g_t = device_planes(GATHER_PLANES, n, dev)
    g_ptrs = {k: v.data_ptr() for k, v in g_t.items()}
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream

    # the pixels' ray directions (the composition faceforwards the normal against them): the hit point minus the eye
    # has the direction's sign on every hit of a pinhole camera
    eye = torch.tensor(list(cam.pos), dtype=torch.float64, device=dev)
    rays_t = torch.empty(n * K * 6, dtype=torch.float64, device=dev)
    w_t = torch.empty(n * K, dtype=torch.float32, device=dev)
    rgb_t = torch.empty(n * K * 3, dtype=torch.float32, device=dev)
    bounce_t = torch.empty(n * 3, dtype=torch.float32, device=dev)
    state = {}

    def c1():
        ctx.renderHitsDevice(cam, opts, hit_ptrs, s)

    def c2_():
        ctx.renderShadingDevice(cam, opts, alb_ptrs, s)

    def c3():
        with torch.cuda.stream(st):
            p = hit_t["p"].view(n, 3)
            state["idx"], state["m"] = build_rays(hit_t["node"], p, hit_t["normal"].view(n, 3), p - eye, K, args.seed, rays_t, w_t)

    def c4():
        m = state["m"]
        for k in range(K):
            ctx.traceRaysDevice(rays_t.data_ptr() + k * m * 48, m, None, rgb_t.data_ptr() + k * m * 12, s)

    def c5():
        with torch.cuda.stream(st):
            reduce_colours(rgb_t, w_t, alb_t["albedo"], state["idx"], state["m"], K, n, bounce_t)

    def fused(planes, k):
        ptrs = {p: g_ptrs[p] for p in planes}
        return lambda: ctx.renderGatherDevice(cam, opts, k, ptrs, seed=args.seed, stream=s)

    # once, untimed: the composition's bounce against the fused call's
    c1(); c2_(); c3(); c4(); c5()
    fused(tuple(GATHER_PLANES), K)()
    torch.cuda.synchronize()
    m = state["m"]
    differ = int((bounce_t.view(n, 3).view(torch.int32) != g_t["bounce"].view(n, 3).view(torch.int32)).any(dim=1).sum())
    lit = int((g_t["bounce"].view(n, 3) != 0).any(dim=1).sum())
    print("%d of %d pixels hit, %d spawned rays, %d pixels with a non-zero bounce; composition against the fused call: %d bounce values differ"
          % (m, n, m * K, lit, differ), flush=True)

    every = tuple(GATHER_PLANES)
    legs = {}
    legs["(a) gather bounce K=%d" % K] = fused(("bounce",), K)
    legs["(b) gather all four K=%d" % K] = fused(every, K)
    legs["(c1) hits node+p+normal"] = c1
    legs["(c2) shading albedo"] = c2_
    legs["(c3) torch: rays"] = c3
    legs["(c4) trace_rays x K"] = c4
    legs["(c5) torch: sums"] = c5
    legs["(d1) gather bounce K=1"] = fused(("bounce",), 1)
    legs["(d64) gather bounce K=64"] = fused(("bounce",), 64)
    legs["(e1) gather all four K=1"] = fused(every, 1)
    legs["(e64) gather all four K=64"] = fused(every, 64)
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
        rows.append({"leg": k, "pixels": n, "hits": m, "samples": K, "us_median": round(med * 1e6, 2), "us_min": round(min(times[k]) * 1e6, 2),
                     "us_max": round(max(times[k]) * 1e6, 2), "windows_us": [round(x * 1e6, 2) for x in times[k]], "passes_per_window": passes[k]})
        print("%-28s %10.1f us [%.1f..%.1f]  (%d passes/window)" % (k, med * 1e6, min(times[k]) * 1e6, max(times[k]) * 1e6, passes[k]), flush=True)
    r = {row["leg"].split(")")[0] + ")": row for row in rows}
    kern = ("(c1)", "(c2)", "(c4)")
    parts = sum(r[k]["us_median"] for k in kern)
    spread = sum(r[k]["us_max"] - r[k]["us_min"] for k in kern)
    whole = parts + r["(c3)"]["us_median"] + r["(c5)"]["us_median"]
    print("(a) = %.1f us against (c1) + (c2) + (c4) = %.1f us (spread of their windows %.1f us): %s;  whole composition %.1f us = %.2f x (a)"
          % (r["(a)"]["us_median"], parts, spread, "met" if r["(a)"]["us_median"] <= parts + spread else "NOT met", whole, whole / r["(a)"]["us_median"]), flush=True)
    print("per sample: fused ((d64) - (d1)) / 63 = %.2f us, composed (c4) / K = %.2f us;  (b) - (a) = %+.1f us" %
          ((r["(d64)"]["us_median"] - r["(d1)"]["us_median"]) / 63, r["(c4)"]["us_median"] / K, r["(b)"]["us_median"] - r["(a)"]["us_median"]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"hits": m, "pixels": n, "bounce_differ": differ, "legs": rows}, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

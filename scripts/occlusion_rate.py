#!/usr/bin/env python3
"""Time per frame of the occlusion planes (c2rt_render_occlusion_device) on lecture5.sdl at 1920x1080, everything resident
in HBM, next to what a caller did for the same planes before the call existed, each part of that timed on its own:

  (a) occlusion ao, K = 16       c2rt_render_occlusion_device, `ao` only
  (b) occlusion all four         node, open, ao, bent
  (c1) hit planes                c2rt_render_hits_device with node, p, normal
  (c2) torch: segments           the K segments of every hit, built on the device from the same counter RNG (48 B x K
                                 per hit written)
  (c3) visibility                c2rt_test_visibility_device over the K x hits segments
  (c4) torch: reduction          answers -> mask and open fraction
  (d1) occlusion ao, K = 1       the cost per sample: (a) at one sample
  (d64) occlusion ao, K = 64     and at 64

The composition's masks are compared with (b)'s `open` once, outside the timed loops, and the number that differ is
printed (torch evaluates the definition's operations one kernel each, so nothing is contracted).

Every timed window holds at least --window-ms of work behind a settling phase and ends in a device sync; the legs are
interleaved --rounds times in one process and the median, minimum and maximum are printed.  The expectation held
against the numbers: (a) <= (c1) + (c3), the allowance being the spread of the windows of those legs.

  python scripts/occlusion_rate.py [--rounds 5] [--json out.json]
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
from chess2rt_amd.api import HIT_PLANES, OCCLUSION_PLANES

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
M32 = 0xFFFFFFFF


def device_planes(table, n, dev):
    return {k: torch.empty(n * comps, dtype=torch.from_numpy(np.empty(0, dtype=t)).dtype, device=dev) for k, (t, comps) in table.items()}


# ---- the definition's sample generator in torch (uint32 arithmetic in int64, masked) ----------------------------------


def hash32(x):
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & M32
    return x ^ (x >> 16)


def rng_key(seed, idx):
    k = hash32(torch.full_like(idx, ((seed >> 32) & M32) ^ 0x243f6a88))
    k = hash32(k ^ (seed & M32))
    k = hash32((k + (idx >> 32)) & M32)
    k = hash32(k ^ (idx & M32))
    return hash32(k)                      # tap 0


def rng_uniform(key, sample, dim):
    h = hash32((key + ((0x9e3779b9 * (sample * 16 + dim + 1)) & M32)) & M32)
    return h.to(torch.float64) * 2.0 ** -32


SIN = [1 / math.factorial(k) * (-1) ** ((k - 1) // 2) for k in (17, 15, 13, 11, 9, 7, 5, 3)]
COS = [1 / math.factorial(k) * (-1) ** (k // 2) for k in (16, 14, 12, 10, 8, 6, 4, 2)]


def sincos2pi(u):
    t = u * 4.0
    q = t.to(torch.int64)
    f = t - q.to(torch.float64)
    mirror = f > 0.5
    g = torch.where(mirror, 1.0 - f, f)
    th = g * (math.pi / 2)
    z = th * th
    ps = torch.full_like(z, SIN[0])
    for c in SIN[1:]:
        ps = c + z * ps
    s = th + th * (z * ps)
    pc = torch.full_like(z, COS[0])
    for c in COS[1:]:
        pc = c + z * pc
    c = 1.0 + z * pc
    a, b = torch.where(mirror, c, s), torch.where(mirror, s, c)
    odd = (q & 1) == 1
    sn, cs = torch.where(odd, b, a), torch.where(odd, a, b)
    sn = torch.where((q == 2) | (q == 3), -sn, sn)
    cs = torch.where((q == 1) | (q == 2), -cs, cs)
    return sn, cs


def build_segments(node, p, normal, d, K, radius, seed, seg_out):
    """the K segments of every hit into seg_out[: hits * K]; returns (indices of the hits, their count)"""
    idx = torch.nonzero(node >= 0).reshape(-1)
    nrm, rd = normal[idx], d[idx]
    front = ((rd[:, 0] * nrm[:, 0] + rd[:, 1] * nrm[:, 1]) + rd[:, 2] * nrm[:, 2]) < 0
    N = torch.where(front[:, None], nrm, -nrm)
    frm = p[idx] + N * 1e-6
    key = rng_key(seed, idx)[:, None]
    s = torch.arange(K, device=node.device, dtype=torch.int64)[None, :]
    u, v = rng_uniform(key, s, 0), rng_uniform(key, s, 1)
    sn, cs = sincos2pi(u)
    w = 2.0 * v - 1.0
    c = torch.sqrt(1.0 - w * w)
    res = torch.stack([cs * c, -w, sn * c], dim=-1)
    flip = ((res[..., 0] * N[:, None, 0] + res[..., 1] * N[:, None, 1]) + res[..., 2] * N[:, None, 2]) < 0
    res = torch.where(flip[..., None], -res, res)
    m = len(idx)
    seg = seg_out[: m * K * 6].view(m, K, 6)
    seg[:, :, :3] = frm[:, None, :]
    seg[:, :, 3:] = frm[:, None, :] + res * radius
    return idx, m


def reduce_answers(vis, idx, m, K, n, open_out, ao_out):
    bits = (vis[: m * K].view(m, K).to(torch.int64) << torch.arange(K, device=vis.device, dtype=torch.int64)[None, :]).sum(dim=1)
    open_out.fill_((1 << K) - 1 if K < 64 else -1)
    open_out[idx] = bits
    ao_out.fill_(1.0)
    ao_out[idx] = vis[: m * K].view(m, K).sum(dim=1).to(torch.float32) / float(K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--radius", type=float, default=120.0)
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
    occ_t = device_planes(OCCLUSION_PLANES, n, dev)
    occ_ptrs = {k: v.data_ptr() for k, v in occ_t.items()}
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream

    # the pixels' ray directions (the composition faceforwards the normal against them): the hit point minus the eye
    # has the direction's sign on every hit of a pinhole camera
    eye = torch.tensor(list(cam.pos), dtype=torch.float64, device=dev)
    seg_t = torch.empty(n * K * 6, dtype=torch.float64, device=dev)
    vis_t = torch.empty(n * K, dtype=torch.uint8, device=dev)
    open_t = torch.empty(n, dtype=torch.int64, device=dev)
    ao_t = torch.empty(n, dtype=torch.float32, device=dev)
    state = {}

    def c1():
        ctx.renderHitsDevice(cam, opts, hit_ptrs, s)

    def c2_():
        with torch.cuda.stream(st):
            p = hit_t["p"].view(n, 3)
            state["idx"], state["m"] = build_segments(hit_t["node"], p, hit_t["normal"].view(n, 3), p - eye, K, args.radius, args.seed, seg_t)

    def c3():
        ctx.testVisibilityDevice(seg_t.data_ptr(), state["m"] * K, vis_t.data_ptr(), s)

    def c4():
        with torch.cuda.stream(st):
            reduce_answers(vis_t, state["idx"], state["m"], K, n, open_t, ao_t)

    def fused(planes, k):
        ptrs = {p: occ_ptrs[p] for p in planes}
        return lambda: ctx.renderOcclusionDevice(cam, opts, k, args.radius, ptrs, seed=args.seed, stream=s)

    # once, untimed: the composition's masks against the fused call's
    c1(); c2_(); c3(); c4()
    fused(tuple(OCCLUSION_PLANES), K)()
    torch.cuda.synchronize()
    m = state["m"]
    differ = int((open_t != occ_t["open"].view(torch.int64)).sum())
    ao_differ = int((ao_t != occ_t["ao"]).sum())
    print("%d of %d pixels hit, %d segments; composition against the fused call: %d masks, %d ao values differ" % (m, n, m * K, differ, ao_differ), flush=True)

    legs = {}
    legs["(a) occlusion ao K=%d" % K] = fused(("ao",), K)
    legs["(b) occlusion all four"] = fused(tuple(OCCLUSION_PLANES), K)
    legs["(c1) hits node+p+normal"] = c1
    legs["(c2) torch: segments"] = c2_
    legs["(c3) visibility"] = c3
    legs["(c4) torch: reduction"] = c4
    legs["(d1) occlusion ao K=1"] = fused(("ao",), 1)
    legs["(d64) occlusion ao K=64"] = fused(("ao",), 64)
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
    parts = r["(c1)"]["us_median"] + r["(c3)"]["us_median"]
    spread = (r["(c1)"]["us_max"] - r["(c1)"]["us_min"]) + (r["(c3)"]["us_max"] - r["(c3)"]["us_min"])
    whole = parts + r["(c2)"]["us_median"] + r["(c4)"]["us_median"]
    print("(a) = %.1f us against (c1) + (c3) = %.1f us (spread of their windows %.1f us): %s;  whole composition %.1f us = %.2f x (b)"
          % (r["(a)"]["us_median"], parts, spread, "met" if r["(a)"]["us_median"] <= parts + spread else "NOT met", whole, whole / r["(b)"]["us_median"]), flush=True)
    print("per sample: ((d64) - (d1)) / 63 = %.2f us;  (b) - (a) = %+.1f us" %
          ((r["(d64)"]["us_median"] - r["(d1)"]["us_median"]) / 63, r["(b)"]["us_median"] - r["(a)"]["us_median"]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"hits": m, "pixels": n, "masks_differ": differ, "ao_differ": ao_differ, "legs": rows}, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

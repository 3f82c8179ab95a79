#!/usr/bin/env python3
"""Time per frame of the path planes (c2rt_render_paths_device) on lecture5.sdl and csg_stress.sdl at 1920x1080 with P = 16
paths, everything resident in HBM:

  (g)  gather, K = P             c2rt_render_gather_device: node, hits, indirect, bounce (the unit the paths grew from)
  (p1) paths, B = 1              c2rt_render_paths_device: node, segments, indirect, bounce — the same work as (g) plus
                                 the cursor's bookkeeping
  (p2) / (p4) paths, B = 2 / 4   the same planes
  (r4) paths, B = 4, all five    with `radiance`: the primary hit's shadow rays on top
  (c1) hit planes                c2rt_render_hits_device with node, p, normal             } the kernels of the route a
  (c2) shading planes            c2rt_render_shading_device with albedo                   } caller had for (p4)'s
  (c4) trace_rays + albedo x B   per depth ONE c2rt_trace_rays_device (records and colours) over the compacted live
                                 paths of all pixels and, where the path goes on, one c2rt_trace_rays_shading_device
                                 (albedo) — B + B - 1 launches, fewer and larger than one per path and depth
  (c3) torch glue                everything else of that route: the rays of every depth from the same counter RNG, the
                                 compaction of the live paths, the throughputs and the ordered fp32 sums

Once, outside the timed loops: (p1)'s `indirect` and `bounce` against (g)'s, (p4)'s `bounce` against the composition's,
pixels that differ printed (zero may differ); and the loop's trip counts per wave (8x8 tile), derived from `segments`:
a lane of a hit traces P + segments(B - 1) segments (every path's first, plus one behind every hit above the last
depth), so the flat loop's trips are the largest such count of the tile; the nest "for path, for bounce" walks, per path,
the deepest any lane of the tile gets, which the difference of `segments` between P' and P' - 1 paths gives per path.

Every timed window holds at least --window-ms of work behind a settling phase and ends in a device sync; the legs are
interleaved --rounds times in one process and the median, minimum and maximum are printed.  A library built with the
nested loop (make VARIANT=nested EXTRA_HIPFLAGS=-DC2RT_PATHS_NESTED, C2RT_LIB_VARIANT=nested) runs the same legs in a
process of its own.

  python scripts/paths_rate.py [--rounds 5] [--scenes lecture5 csg_stress] [--no-composed] [--json out.json]
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
from chess2rt_amd.api import GATHER_PLANES, HIT_PLANES, PATH_PLANES, SHADE_PLANES
from occlusion_rate import M32, SCENES, device_planes, hash32, rng_uniform, sincos2pi   # the definition's sample generator in torch


def rng_key(seed, idx, tap):
    k = hash32(torch.full_like(idx, ((seed >> 32) & M32) ^ 0x243f6a88))
    k = hash32(k ^ (seed & M32))
    k = hash32((k + (idx >> 32)) & M32)
    k = hash32(k ^ (idx & M32))
    return hash32((k + tap) & M32)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def faceforward(d, n):
    return torch.where((dot3(d, n) < 0)[:, None], n, -n)


def directions(seed, idx, j, path, N):
    key = rng_key(seed, idx, j)
    u, v = rng_uniform(key, path, 0), rng_uniform(key, path, 1)
    sn, cs = sincos2pi(u)
    w = 2.0 * v - 1.0
    c = torch.sqrt(1.0 - w * w)
    res = torch.stack([cs * c, -w, sn * c], dim=-1)
    return torch.where((dot3(res, N) < 0)[:, None], -res, res)


class Composed:
    """the route a caller had: the library's single-purpose queries, torch in between; kernels and glue timed apart"""

    def __init__(self, ctx, cam, opts, n, P, B, seed, dev, stream):
        self.ctx, self.cam, self.opts, self.n, self.P, self.B, self.seed, self.st = ctx, cam, opts, n, P, B, seed, stream
        self.hit_t = device_planes({k: HIT_PLANES[k] for k in ("node", "p", "normal")}, n, dev)
        self.alb_t = device_planes({"albedo": SHADE_PLANES["albedo"]}, n, dev)
        self.eye = torch.tensor(list(cam.pos), dtype=torch.float64, device=dev)
        self.rays = torch.empty(n * P * 6, dtype=torch.float64, device=dev)
        self.rec = torch.empty(n * P * 10, dtype=torch.float64, device=dev)     # c2rt_ray_hit: ten 8-byte words
        self.rgb = torch.empty(n * P * 3, dtype=torch.float32, device=dev)
        self.alb = torch.empty(n * P * 3, dtype=torch.float32, device=dev)
        self.bounce = torch.zeros(n * 3, dtype=torch.float32, device=dev)
        self.t_kernels = self.t_glue = 0.0

    def _timed(self, kernels, fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        if kernels:
            self.t_kernels += dt
        else:
            self.t_glue += dt
        return out

    def run(self):
        """one frame's `bounce`; adds to t_kernels / t_glue (a sync around every part: an upper bound on both)"""
        ctx, s, n, P, B = self.ctx, self.st.cuda_stream, self.n, self.P, self.B
        self._timed(True, lambda: ctx.renderHitsDevice(self.cam, self.opts, {k: v.data_ptr() for k, v in self.hit_t.items()}, s))
        self._timed(True, lambda: ctx.renderShadingDevice(self.cam, self.opts, {"albedo": self.alb_t["albedo"].data_ptr()}, s))

        def start():
            with torch.cuda.stream(self.st):
                pix = torch.nonzero(self.hit_t["node"] >= 0).reshape(-1)
                p = self.hit_t["p"].view(n, 3)[pix]
                N0 = faceforward(p - self.eye, self.hit_t["normal"].view(n, 3)[pix])
                m = len(pix)
                slot = torch.arange(m, device=pix.device).repeat_interleave(P)      # pixel-major, path-minor
                path = torch.arange(P, device=pix.device).repeat(m)
                term = torch.zeros(m, P, B, 3, dtype=torch.float32, device=pix.device)
                return pix, m, slot, path, N0[slot], (p + N0 * 1e-6)[slot], term
        pix, m, slot, path, N, frm, term = self._timed(False, start)
        T = None
        for j in range(B):
            def spawn():
                with torch.cuda.stream(self.st):
                    res = directions(self.seed, pix[slot], j, path, N)
                    w = (2.0 * dot3(res, N)).to(torch.float32)
                    k = len(slot)
                    r = self.rays[: k * 6].view(k, 6)
                    r[:, :3] = frm
                    r[:, 3:] = res
                    return res, w, k
            res, w, k = self._timed(False, spawn)
            if k == 0:
                break
            self._timed(True, lambda: ctx.traceRaysDevice(self.rays.data_ptr(), k, self.rec.data_ptr(), self.rgb.data_ptr(), s))
            more = j + 1 < B
            if more:
                self._timed(True, lambda: ctx.traceRaysShadingDevice(self.rays.data_ptr(), k, {"albedo": self.alb.data_ptr()}, s))

            def advance():
                nonlocal T
                with torch.cuda.stream(self.st):
                    T = w[:, None].expand(k, 3) if j == 0 else T * w[:, None]
                    term[slot, path, j] = self.rgb[: k * 3].view(k, 3) * T
                    if not more:
                        return None
                    rec = self.rec[: k * 10].view(k, 10)
                    on = torch.nonzero((rec[:, 0].view(torch.int64) & M32) < 0x80000000).reshape(-1)   # closest_node >= 0
                    T = (T * self.alb[: k * 3].view(k, 3))[on]
                    Nn = faceforward(res[on], rec[on, 7:10])
                    return slot[on], path[on], Nn, rec[on, 4:7] + Nn * 1e-6
            nxt = self._timed(False, advance)
            if nxt is None:
                break
            slot, path, N, frm = nxt

        def reduce():
            with torch.cuda.stream(self.st):
                total = torch.zeros(m, 3, dtype=torch.float32, device=pix.device)
                for p_ in range(P):
                    for j in range(B):
                        total = total + term[:, p_, j]     # a path that ended adds +0: the bits of the sum stay
                self.bounce.zero_()
                self.bounce.view(n, 3)[pix] = self.alb_t["albedo"].view(n, 3)[pix] * (total / float(P))
        self._timed(False, reduce)
        return m


def trips(ctx, cam, opts, n, w, h, P, B, seed, stream, dev):
    """(flat, nested) trip counts per 8x8 tile, derived from `segments`"""
    seg = torch.empty(n, dtype=torch.int32, device=dev)
    node = torch.empty(n, dtype=torch.int32, device=dev)

    def segments(paths, bounces):
        ctx.renderPathsDevice(cam, opts, paths, bounces, {"segments": seg.data_ptr(), "node": node.data_ptr()}, seed=seed, stream=stream.cuda_stream)
        stream.synchronize()
        return seg.clone().to(torch.int64)

    def tiles(x):   # max over the lanes of every 8x8 tile
        hp, wp = -(-h // 8) * 8, -(-w // 8) * 8
        full = torch.zeros(hp, wp, dtype=x.dtype, device=dev)
        full[:h, :w] = x.view(h, w)
        return full.view(hp // 8, 8, wp // 8, 8).amax(dim=(1, 3)).reshape(-1)

    below = segments(P, B - 1) if B > 1 else torch.zeros(n, dtype=torch.int64, device=dev)
    hit = node >= 0
    flat = tiles(torch.where(hit, P + below, torch.zeros_like(below)))
    nested = torch.zeros_like(flat)
    prev = torch.zeros(n, dtype=torch.int64, device=dev)
    for paths in range(1, P + 1):
        cur = segments(paths, B)
        depth = torch.where(hit, torch.clamp(cur - prev + 1, max=B), torch.zeros_like(cur))   # segments traced by path paths - 1
        nested += tiles(depth)
        prev = cur
    return flat.to(torch.float64), nested.to(torch.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--paths", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--scenes", nargs="+", default=["lecture5", "csg_stress"])
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--no-trips", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    w, h = args.size
    n, P = w * h, args.paths
    dev = torch.device("cuda:0")
    ctx = c2.Context(0)
    report = {"variant": os.environ.get("C2RT_LIB_VARIANT", ""), "scenes": {}}
    print("library variant: %r" % report["variant"], flush=True)
    for name in args.scenes:
        scene = c2.parseSceneFromFile(os.path.join(SCENES, name + ".sdl"))
        scene.setFrameSize(w, h)
        scene.setAA(False)
        scene.setDof(False)
        cam = scene.beginFrame()
        opts = scene.renderOpts(taps=1)
        ctx.uploadScene(scene.desc)
        st = torch.cuda.Stream(dev)
        s = st.cuda_stream
        g_t = device_planes(GATHER_PLANES, n, dev)
        p_t = device_planes(PATH_PLANES, n, dev)
        four = ("node", "segments", "indirect", "bounce")

        def gather():
            ctx.renderGatherDevice(cam, opts, P, {k: v.data_ptr() for k, v in g_t.items()}, seed=args.seed, stream=s)

        def paths(bounces, planes):
            ptrs = {k: p_t[k].data_ptr() for k in planes}
            return lambda: ctx.renderPathsDevice(cam, opts, P, bounces, ptrs, seed=args.seed, stream=s)

        # once, untimed: one bounce against the gather planes
        gather()
        paths(1, four)()
        torch.cuda.synchronize()
        hits = int((p_t["node"] >= 0).sum())
        differ = {k: int((g_t[k].view(n, 3).view(torch.int32) != p_t[k].view(n, 3).view(torch.int32)).any(dim=1).sum()) for k in ("indirect", "bounce")}
        print("%s %dx%d, P = %d: %d of %d pixels hit; paths B = 1 against the gather planes: %d indirect, %d bounce values differ"
              % (name, w, h, P, hits, n, differ["indirect"], differ["bounce"]), flush=True)
        out = {"pixels": n, "hits": hits, "gather_differ": differ}
        if not args.no_trips:
            for B in (2, 4):
                flat, nested = trips(ctx, cam, opts, n, w, h, P, B, args.seed, st, dev)
                live = flat > 0
                out["trips_B%d" % B] = {"tiles": int(live.sum()), "flat_mean": float(flat[live].mean()), "flat_max": float(flat.max()),
                                        "nested_mean": float(nested[live].mean()), "nested_max": float(nested.max())}
                print("  B = %d, iterations per wave over the %d tiles with a hit: flat mean %.1f max %d, nested mean %.1f max %d (bound %d)"
                      % (B, int(live.sum()), out["trips_B%d" % B]["flat_mean"], int(flat.max()), out["trips_B%d" % B]["nested_mean"], int(nested.max()), P * B), flush=True)
        if not args.no_composed:
            comp = Composed(ctx, cam, opts, n, P, 4, args.seed, dev, st)
            comp.run()                                             # warm
            comp.t_kernels = comp.t_glue = 0.0
            reps = 3
            for _ in range(reps):
                comp.run()
            paths(4, four)()
            torch.cuda.synchronize()
            cdiff = int((comp.bounce.view(n, 3).view(torch.int32) != p_t["bounce"].view(n, 3).view(torch.int32)).any(dim=1).sum())
            out["composed"] = {"kernels_us": comp.t_kernels / reps * 1e6, "glue_us": comp.t_glue / reps * 1e6, "bounce_differ": cdiff}
            print("  composed route, B = 4: kernels alone %.1f us, torch glue %.1f us (mean of %d, a sync around every part); its bounce against the fused call's: %d values differ"
                  % (out["composed"]["kernels_us"], out["composed"]["glue_us"], reps, cdiff), flush=True)
            del comp
            torch.cuda.empty_cache()

        legs = {"(g) gather K=%d" % P: gather, "(p1) paths B=1": paths(1, four), "(p2) paths B=2": paths(2, four), "(p4) paths B=4": paths(4, four),
                "(r4) paths B=4 all five": paths(4, tuple(PATH_PLANES))}
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
        rows = {}
        for k in legs:
            med = statistics.median(times[k])
            rows[k.split(")")[0] + ")"] = {"leg": k, "us_median": round(med * 1e6, 2), "us_min": round(min(times[k]) * 1e6, 2), "us_max": round(max(times[k]) * 1e6, 2),
                                           "windows_us": [round(x * 1e6, 2) for x in times[k]], "passes_per_window": passes[k]}
            print("  %-26s %10.1f us [%.1f..%.1f]  (%d passes/window)" % (k, med * 1e6, min(times[k]) * 1e6, max(times[k]) * 1e6, passes[k]), flush=True)
        g, p1 = rows["(g)"], rows["(p1)"]
        allowance = (g["us_max"] - g["us_min"]) + 0.05 * g["us_median"]
        print("  (p1) = %.1f us against (g) = %.1f us + its window spread %.1f us + 5 %% = %.1f us: %s (%+.1f %%)"
              % (p1["us_median"], g["us_median"], g["us_max"] - g["us_min"], g["us_median"] + allowance,
                 "met" if p1["us_median"] <= g["us_median"] + allowance else "NOT met", (p1["us_median"] / g["us_median"] - 1) * 100), flush=True)
        if "composed" in out:
            print("  (p4) = %.1f us against the composed route's kernels alone %.1f us: %.2f x" % (rows["(p4)"]["us_median"], out["composed"]["kernels_us"],
                                                                                               out["composed"]["kernels_us"] / rows["(p4)"]["us_median"]), flush=True)
        out["legs"] = rows
        report["scenes"][name] = out
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

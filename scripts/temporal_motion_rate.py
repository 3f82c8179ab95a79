#!/usr/bin/env python3
"""Time of the accumulation that follows moved nodes (c2rt_temporal_accumulate_motion_device) on lecture5.sdl, three
channels, everything resident in HBM — scripts/temporal_rate.py's set-up: the guides are the context's own hit planes of a
camera one small step past the camera whose frame left the history, the input is the path planes' `indirect`.

  (i)    the motion entry with ONE listed node that covers a small part of the frame (the hit node with the fewest pixels)
  (ii)   the motion entry with EVERY hit node listed: every hit pixel goes through its record
  (iii)  the static entry, c2rt_temporal_accumulate_device, of the same build
  (y)    the yardstick: c2rt_temporal_accumulate_device of --yardstick NAME (chess2rt_amd/libc2rt_NAME.so, a build of the
         commit before the motion entry existed), loaded into the same process

Every listed node's two poses are the same one, so that the motion is coherent and the planes comparable: the records are
the identity and a moved lane does all of its work — the loads of its record, the two carries, the squared tests — on
values that leave its point where it was.  (iii) must hold the bits of (y); (i) and (ii) hold them too but for taps whose
squared tests round the other way at a threshold; the script counts the bytes that differ before it times anything.

--variants a,b adds the motion entry of libc2rt_a.so, libc2rt_b.so (builds that differ in how the kernel reads its
records) as further legs of (i) and (ii).  Every window holds --calls calls behind a warm-up and lies between two device
events; all legs are interleaved --rounds times in one process; median [min..max] per call, and every ratio taken round by
round.

  python scripts/temporal_motion_rate.py [--sizes 1920x1080,3840x2160] [--rounds 9] [--calls 20] [--yardstick parent] [--variants tab] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import chess2rt_amd as c2
from chess2rt_amd import _abi

MIN_NORMAL_DOT, MAX_PLANE_DIST, MAX_AGE = 0.9, 0.1, 32
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1] * 3 + [0, 0, 0], dtype=np.float64)


def med(v):
    return "%9.1f us [%.1f..%.1f]" % (statistics.median(v), min(v), max(v))


class Lib:
    """a build of the library and a context of its own on device 0 (no name: the package's)"""

    def __init__(self, variant, motion=True):
        self.name = variant or "libc2rt"
        if variant:
            self.lib = C.CDLL(os.path.join(ROOT, "chess2rt_amd", "libc2rt_%s.so" % variant), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # DEEPBIND: its own launchers
            for name in ("c2rt_init", "c2rt_destroy", "c2rt_last_error", "c2rt_temporal_accumulate_device") + (("c2rt_temporal_accumulate_motion_device",) if motion else ()):
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = _abi.C2RT_SYMBOLS[name]
        else:
            self.lib = _abi.load_library()
        self.h = C.c_void_p()
        assert self.lib.c2rt_init(0, C.byref(self.h)) == 0

    def static(self, cam, g, o, src, prev, out, planes, stream):
        st = self.lib.c2rt_temporal_accumulate_device(self.h, C.byref(cam), C.byref(g), C.byref(o), src, prev, out, C.byref(planes), stream)
        assert st == 0, self.lib.c2rt_last_error(self.h)

    def motion(self, cam, g, o, m, src, prev, out, planes, stream):
        st = self.lib.c2rt_temporal_accumulate_motion_device(self.h, C.byref(cam), C.byref(g), C.byref(o), C.byref(m), src, prev, out, C.byref(planes), stream)
        assert st == 0, self.lib.c2rt_last_error(self.h)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--paths", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--yardstick", default="parent")
    ap.add_argument("--variants", default="")
    ap.add_argument("--json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    ctx = c2.Context(0)
    own, yard = Lib(""), Lib(a.yardstick, motion=False)
    variants = [Lib(v) for v in a.variants.split(",") if v]
    result = {"sizes": {}}
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        px = W * H
        scene = c2.parseSceneFromFile(os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl"))
        scene.setFrameSize(W, H)
        scene.setAA(False)
        scene.setDof(False)
        opts = scene.renderOpts(taps=_abi.TAPS_1)
        cams = [scene.beginFrame()]
        scene.moveCamera(1.0, 0.2, 0.5)
        scene.rotateCamera(0.8, 0.0, 0.3)
        cams.append(scene.beginFrame())
        ctx.uploadScene(scene.desc)

        def planes_of(cam, seed):
            t = dict(node=torch.empty((H, W), dtype=torch.int32, device=dev), normal=torch.empty((H, W, 3), dtype=torch.float64, device=dev),
                     p=torch.empty((H, W, 3), dtype=torch.float64, device=dev), indirect=torch.empty((H, W, 3), dtype=torch.float32, device=dev))
            ctx.renderHitsDevice(cam, opts, {k: t[k].data_ptr() for k in ("node", "normal", "p")}, stream=stream)
            ctx.renderPathsDevice(cam, opts, a.paths, a.bounces, {"indirect": t["indirect"].data_ptr()}, seed=seed, stream=stream)
            torch.cuda.synchronize()
            return t

        f0, f1 = planes_of(cams[0], 7), planes_of(cams[1], 8)
        nodes, counts = torch.unique(f1["node"][f1["node"] >= 0], return_counts=True)
        nodes, counts = nodes.tolist(), counts.tolist()
        small = nodes[counts.index(min(counts))]
        hit = sum(counts)
        print("lecture5 %dx%d: %d of %d pixels hit, on nodes %s; the small node %d covers %d pixels (%.2f %% of the frame)"
              % (W, H, hit, px, dict(zip(nodes, counts)), small, min(counts), 100.0 * min(counts) / px))

        def motion_of(listed):
            idx = np.array(listed, dtype=np.uint32)
            xf = np.ascontiguousarray(np.tile(IDENTITY, (len(listed), 1)))
            m = _abi.TemporalMotion(n_nodes=len(listed), node_index=idx.ctypes.data_as(_abi._u32p), prev_transform=xf.ctypes.data_as(_abi._f64p),
                                    cur_transform=xf.ctypes.data_as(_abi._f64p))
            m._keep = (idx, xf)
            return m

        m_one, m_all = motion_of([small]), motion_of(nodes)
        o = _abi.TemporalOpts(width=W, height=H, channels=3, max_age=MAX_AGE, min_normal_dot=MIN_NORMAL_DOT, max_plane_dist=MAX_PLANE_DIST)
        need = c2.temporal_history_bytes(W, H, 3)
        g0 = _abi.TemporalGuides(node=f0["node"].data_ptr(), normal=f0["normal"].data_ptr(), p=f0["p"].data_ptr())
        g1 = _abi.TemporalGuides(node=f1["node"].data_ptr(), normal=f1["normal"].data_ptr(), p=f1["p"].data_ptr())
        prev = torch.empty(need, dtype=torch.uint8, device=dev)
        st = own.lib.c2rt_temporal_accumulate_device(own.h, None, C.byref(g0), C.byref(o), f0["indirect"].data_ptr(), None, prev.data_ptr(),
                                                      C.byref(_abi.TemporalPlanes()), stream)
        assert st == 0

        def buffers():
            buf = dict(hist=torch.empty(need, dtype=torch.uint8, device=dev), colour=torch.empty((H, W, 3), dtype=torch.float32, device=dev),
                       variance=torch.empty((H, W), dtype=torch.float32, device=dev), age=torch.empty((H, W), dtype=torch.int32, device=dev))
            buf["planes"] = _abi.TemporalPlanes(colour=buf["colour"].data_ptr(), variance=buf["variance"].data_ptr(), age=buf["age"].data_ptr())
            return buf

        # the legs: (label, library, motion or None), each with outputs of its own
        legs = [("i one small node", own, m_one), ("ii every hit node", own, m_all), ("iii static", own, None), ("y yardstick static (%s)" % yard.name, yard, None)]
        for v in variants:
            legs += [("i one small node, %s" % v.name, v, m_one), ("ii every hit node, %s" % v.name, v, m_all)]
        bufs = [buffers() for _ in legs]

        def run(k):
            _, lib, m = legs[k]
            b = bufs[k]
            if m is None:
                lib.static(cams[0], g1, o, f1["indirect"].data_ptr(), prev.data_ptr(), b["hist"].data_ptr(), b["planes"], stream)
            else:
                lib.motion(cams[0], g1, o, m, f1["indirect"].data_ptr(), prev.data_ptr(), b["hist"].data_ptr(), b["planes"], stream)

        for k in range(len(legs)):
            run(k)
        torch.cuda.synchronize()
        ref = bufs[3]
        for k, (label, _, _) in enumerate(legs):
            differ = sum(int((bufs[k][n].view(torch.uint8) != ref[n].view(torch.uint8)).sum()) for n in ("hist", "colour", "variance", "age"))
            print("  (%s) against the yardstick: %d bytes of planes and history differ" % (label, differ))
            assert differ == 0 or legs[k][2] is not None, label            # a moved lane's squared tests may round another way at a threshold
        age = ref["age"]
        print("  %d pixels found their history (age 2), %d restarted, %d missed" % (int((age == 2).sum()), int((age == 1).sum()), int((age == 0).sum())))

        T = [[] for _ in legs]
        for _ in range(a.rounds):
            for k in range(len(legs)):
                T[k].append(window(lambda: run(k), a.calls))
        entry = {}
        for k, (label, _, _) in enumerate(legs):
            ratio = [x / y for x, y in zip(T[k], T[3])]
            print("  (%-32s) %s   over the yardstick, round by round: %.3f [%.3f..%.3f]" % (label, med(T[k]), statistics.median(ratio), min(ratio), max(ratio)))
            entry[label] = {"us": T[k], "over_yardstick": ratio}
        for k in range(4, len(legs)):
            ratio = [x / y for x, y in zip(T[k], T[(k - 4) % 2])]
            print("  (%s) over this build's, round by round: %.3f [%.3f..%.3f]" % (legs[k][0], statistics.median(ratio), min(ratio), max(ratio)))
        result["sizes"][size] = entry
        del bufs, f0, f1, prev
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A global-illumination frame of a scene's camera through Context.renderPaths: one call, one launch, and every pixel's
closest hit comes back with the light that reaches it over up to maxTraceDepth bounces — renderSampleGI's frame
(rt/renderer.d:289-301) in the build-defined reading of include/c2rt.h.  The script writes the one-tap frame as it is
(<stem>_direct.bmp), the one-bounce frame (<stem>_gi1.bmp: direct + the `bounce` plane at bounces = 1, the gather
planes' frame) and the `radiance` plane at the scene's own depth (<stem>_gi.bmp), and prints the mean `bounce` of the
hits for bounces = 1 .. maxTraceDepth: what every further bounce adds.

  python examples/render_gi.py tests/golden/scenes/lecture5.sdl /tmp/gi --size 640 480 --paths 16
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chess2rt_amd as c2


def write(path, image):
    with open(path, "wb") as f:
        f.write(c2.saveBmp(np.ascontiguousarray(image, dtype=np.float32)))
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("stem", help="the images are written as <stem>_<pass>.bmp")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=(640, 480))
    ap.add_argument("--paths", type=int, default=None, help="paths per pixel, 1 .. 64 (default: the scene's pathsPerPixel, at most 64)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    scene.setFrameSize(*args.size)
    scene.setAA(False)
    scene.setDof(False)                                  # a pixel's paths are one ray's: no lens
    s = scene.settings
    paths = min(s.paths_per_pixel, 64) if args.paths is None else args.paths
    depth = max(1, min(s.max_trace_depth, 8))
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    cam, opts = scene.beginFrame(), scene.renderOpts()
    direct = ctx.renderHits(cam, opts, planes=("node", "rgb"))
    hit = direct["node"] >= 0
    means = []
    for b in range(1, depth + 1):
        pl = ctx.renderPaths(cam, opts, paths, b, seed=args.seed, planes=("bounce", "radiance", "segments"))
        means.append([round(float(x), 4) for x in pl["bounce"][hit].mean(axis=0)] if hit.any() else [0, 0, 0])
        if b == 1:
            first = pl
    files = [write(args.stem + "_direct.bmp", direct["rgb"]), write(args.stem + "_gi1.bmp", first["radiance"]), write(args.stem + "_gi.bmp", pl["radiance"])]
    print("%s: %dx%d, %d paths, max_trace_depth %d: %d of %d pixels hit, %.2f hitting segments per hit at depth %d"
          % (scene.name, args.size[0], args.size[1], paths, s.max_trace_depth, int(hit.sum()), hit.size,
             float(pl["segments"][hit].mean()) if hit.any() else 0.0, depth))
    for b, m in enumerate(means, 1):
        print("  bounces = %d: mean bounce of the hits %s" % (b, m))
    print("\n".join(files))


if __name__ == "__main__":
    main()

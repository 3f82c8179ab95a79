#!/usr/bin/env python3
"""A global-illumination frame at a path count people actually run, raw and denoised.  Sixteen paths per pixel leave the
path planes' `radiance` speckled; Context.renderPathsDenoised renders the same planes on the device, runs the a-trous
filter over the `indirect` plane alone — guided by the hit planes' node, normal and point, so that it never blurs across
an object's outline, a crease or a step in depth — and multiplies the albedo back in and adds the direct frame after the
filter: textures and shadows stay as sharp as the one-tap frame has them.  The script writes <stem>_raw.bmp and
<stem>_denoised.bmp and prints how much of the pixel-to-pixel variation of the indirect light the filter removed.

  python examples/render_denoised.py tests/golden/scenes/lecture5.sdl /tmp/gi --size 640 480 --paths 16
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


def roughness(image, hit):
    """mean absolute difference between horizontal neighbours that are both hits"""
    both = hit[:, 1:] & hit[:, :-1]
    return float(np.abs(image[:, 1:] - image[:, :-1])[both].mean()) if both.any() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("stem", help="the images are written as <stem>_raw.bmp and <stem>_denoised.bmp")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=(640, 480))
    ap.add_argument("--paths", type=int, default=16)
    ap.add_argument("--levels", type=int, default=5, help="filter passes, 0 .. 8; pass l taps 2^l pixels apart")
    ap.add_argument("--sigma-plane", type=float, default=1.0, help="distance from the centre's tangent plane at which a tap weighs half")
    ap.add_argument("--sigma-colour", type=float, default=0.0, help="colour difference at which a tap weighs half at level 0 (0: no colour term)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    scene.setFrameSize(*args.size)
    scene.setAA(False)
    scene.setDof(False)
    depth = max(1, min(scene.settings.max_trace_depth, 8))
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    cam, opts = scene.beginFrame(), scene.renderOpts()
    raw = ctx.renderPaths(cam, opts, args.paths, depth, seed=args.seed, planes=("node", "indirect", "radiance"))
    denoised = ctx.renderPathsDenoised(cam, opts, args.paths, depth, seed=args.seed, levels=args.levels, sigma_plane=args.sigma_plane,
                                       sigma_colour=args.sigma_colour)
    # the filtered indirect plane by itself, for the figure below: the same call composed by hand
    guides = ctx.renderHits(cam, opts, planes=("node", "normal", "p"))
    smooth = ctx.denoise(guides, raw["indirect"], levels=args.levels, sigma_plane=args.sigma_plane, sigma_colour=args.sigma_colour)
    hit = raw["node"] >= 0
    before, after = roughness(raw["indirect"], hit), roughness(smooth, hit)
    print("%s: %dx%d, %d paths x %d bounces, %d levels: neighbour-to-neighbour difference of the indirect light %.4f -> %.4f (%.0f %% removed)"
          % (scene.name, args.size[0], args.size[1], args.paths, depth, args.levels, before, after, 100.0 * (1.0 - after / before) if before else 0.0))
    print(write(args.stem + "_raw.bmp", raw["radiance"]))
    print(write(args.stem + "_denoised.bmp", denoised))


if __name__ == "__main__":
    main()

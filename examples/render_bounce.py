#!/usr/bin/env python3
"""One-bounce indirect light of a scene's camera through Context.renderGather: one call, one launch, and every pixel's
closest hit comes back with the light it receives from the lit surfaces around it — the floor's bitmap bleeding onto
the balls, a cavity glowing from its own walls.  The script writes the one-tap frame as it is (<stem>_direct.bmp), the
`bounce` plane (<stem>_bounce.bmp: albedo times the mean weighted colour arriving over the hemisphere) and their sum
(<stem>_gi.bmp), a one-bounce global-illumination frame.

  python examples/render_bounce.py tests/golden/scenes/lecture5.sdl /tmp/gi --size 640 480 --samples 16
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
    ap.add_argument("--samples", type=int, default=16, help="spawned rays per pixel, 1 .. 64")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    scene.setFrameSize(*args.size)
    scene.setAA(False)
    scene.setDof(False)                                  # a pixel's gather is one ray's: no lens
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    cam, opts = scene.beginFrame(), scene.renderOpts()
    g = ctx.renderGather(cam, opts, args.samples, seed=args.seed)
    direct = ctx.renderHits(cam, opts, planes=("node", "rgb"))
    assert np.array_equal(g["node"], direct["node"])
    hit = g["node"] >= 0
    assert not g["bounce"][~hit].any() and not g["hits"][~hit].any()
    with np.errstate(invalid="ignore", over="ignore"):
        total = (direct["rgb"] + g["bounce"]).astype(np.float32)
    files = [write(args.stem + "_direct.bmp", direct["rgb"]), write(args.stem + "_bounce.bmp", g["bounce"]), write(args.stem + "_gi.bmp", total)]
    seen = np.array([bin(int(x)).count("1") for x in g["hits"].reshape(-1)]).reshape(hit.shape)
    print("%s: %dx%d, %d samples: %d of %d pixels hit, %.1f %% of their spawned rays hit a surface, mean bounce of the hits %s, mean direct %s"
          % (scene.name, args.size[0], args.size[1], args.samples, int(hit.sum()), hit.size,
             100.0 * float(seen[hit].mean()) / args.samples if hit.any() else 0.0,
             [round(float(x), 4) for x in g["bounce"][hit].mean(axis=0)] if hit.any() else [0, 0, 0],
             [round(float(x), 4) for x in direct["rgb"][hit].mean(axis=0)] if hit.any() else [0, 0, 0]))
    print("\n".join(files))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""An x-ray and a thickness map of a scene's camera through ONE Context.renderHitLayers call (depth peeling: layer k of
a pixel is the k-th surface along its ray).

  x-ray      every surface composited front to back at --opacity: the cavity of lecture5's carved cube and the ground
             behind the spheres show through
  thickness  the length the ray spends between surface pairs — the sum of dist[2j + 1] - dist[2j] over the pairs
             inside `count` — as grey (thickest = white); for a closed solid seen from outside that is the length inside it

  python examples/render_xray.py tests/golden/scenes/lecture5.sdl /tmp/xray.bmp /tmp/thickness.bmp --size 640 480
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chess2rt_amd as c2


def xray_image(rgb, count, opacity):
    """front-to-back 'over' of the layers that are hits: layer k means something for k < count"""
    out = np.zeros(rgb.shape[1:], dtype=np.float32)
    through = np.ones(count.shape, dtype=np.float32)            # what still passes the layers in front
    for k in range(rgb.shape[0]):
        there = (k < count)[..., None]
        out += np.where(there, rgb[k] * (through * opacity)[..., None], 0.0).astype(np.float32)
        through = np.where(there[..., 0], through * (1.0 - opacity), through).astype(np.float32)
    return out


def thickness_map(dist, count):
    thick = np.zeros(count.shape, dtype=np.float64)
    for j in range(dist.shape[0] // 2):
        pair = count >= 2 * j + 2
        thick += np.where(pair, dist[2 * j + 1] - dist[2 * j], 0.0)
    return thick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("xray_bmp")
    ap.add_argument("thickness_bmp")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=(640, 480))
    ap.add_argument("--layers", type=int, default=8, help="surfaces per pixel at most (1 .. %d)" % c2._abi.MAX_HIT_LAYERS)
    ap.add_argument("--opacity", type=float, default=0.5)
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    scene.setFrameSize(*args.size)
    scene.setDof(False)                                  # a pixel's layers are one ray's: no lens
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    pl = ctx.renderHitLayers(scene.beginFrame(), scene.renderOpts(), args.layers, planes=("dist", "rgb"))
    count = pl["count"]
    with np.errstate(invalid="ignore", over="ignore"):
        xray = xray_image(pl["rgb"], count, np.float32(args.opacity))
        thick = thickness_map(pl["dist"], count)
    grey = (thick / max(thick.max(), 1e-300)).astype(np.float32)
    with open(args.xray_bmp, "wb") as f:
        f.write(c2.saveBmp(xray))
    with open(args.thickness_bmp, "wb") as f:
        f.write(c2.saveBmp(np.repeat(grey[..., None], 3, axis=2)))
    print("%s: %dx%d, up to %d surfaces per pixel (%s pixels with 0, 1, 2, ... surfaces), thickest %.4g -> %s, %s" %
          (scene.name, args.size[0], args.size[1], int(count.max()), np.bincount(count.ravel()).tolist(), thick.max(), args.xray_bmp, args.thickness_bmp))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A 360-degree equirectangular panorama from the scene's camera position — a camera the library does not have —
through Context.traceRays: the caller builds one ray per pixel, the GPU traces and shades them.

  python examples/render_panorama.py tests/golden/scenes/lecture5.sdl /tmp/pano.bmp --size 1024 512
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chess2rt_amd as c2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out_bmp")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=(1024, 512))
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    w, h = args.size
    lon = (np.arange(w) + 0.5) / w * 2 * np.pi - np.pi          # -pi .. pi, left to right
    lat = np.pi / 2 - (np.arange(h) + 0.5) / h * np.pi          # +pi/2 (up) .. -pi/2
    lon, lat = np.meshgrid(lon, lat)
    dirs = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], axis=-1).reshape(-1, 3)
    rays = np.hstack([np.broadcast_to(list(scene.camera.pos), dirs.shape), dirs])   # unit directions, used as given
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    _, rgb = ctx.traceRays(rays, hits=False)
    with open(args.out_bmp, "wb") as f:
        f.write(c2.saveBmp(rgb.reshape(h, w, 3)))
    print("%s: %dx%d panorama, %d rays" % (scene.name, w, h, len(rays)))


if __name__ == "__main__":
    main()

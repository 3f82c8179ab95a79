#!/usr/bin/env python3
"""Depth and node-id images of a scene's camera through Context.renderHits: one call, two of the seven hit planes.
Depth is scaled to grey (near = white, the farthest hit = dark, no hit = black); every node gets a colour of its own.

  python examples/render_depth.py tests/golden/scenes/lecture5.sdl /tmp/depth.bmp /tmp/nodes.bmp --size 640 480
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
    ap.add_argument("depth_bmp")
    ap.add_argument("nodes_bmp")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=(640, 480))
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    scene.setFrameSize(*args.size)
    scene.setDof(False)                                  # a pixel's record is one ray's: no lens
    cam = scene.beginFrame()
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    pl = ctx.renderHits(cam, scene.renderOpts(), planes=("node", "dist"))
    node, dist = pl["node"], pl["dist"]
    hit = node >= 0
    grey = np.zeros(node.shape, dtype=np.float32)
    if hit.any():
        near, far = dist[hit].min(), dist[hit].max()
        grey[hit] = (1.0 - 0.9 * (dist[hit] - near) / max(far - near, 1e-300)).astype(np.float32)
    with open(args.depth_bmp, "wb") as f:
        f.write(c2.saveBmp(np.repeat(grey[..., None], 3, axis=2)))
    # a fixed, well separated colour per node: hues by the golden ratio
    n_nodes = scene.desc.contents.n_nodes
    hue = (np.arange(n_nodes) * 0.618033988749895) % 1.0
    k = (hue[:, None] * 6.0 + np.array([5.0, 3.0, 1.0])) % 6.0
    palette = (1.0 - 0.75 * np.clip(np.minimum(k, 4.0 - k), 0.0, 1.0)).astype(np.float32)
    ids = np.zeros(node.shape + (3,), dtype=np.float32)
    ids[hit] = palette[node[hit]]
    with open(args.nodes_bmp, "wb") as f:
        f.write(c2.saveBmp(ids))
    print("%s: %dx%d, %d of %d pixels hit, %d nodes seen" % (scene.name, args.size[0], args.size[1], int(hit.sum()), node.size, len(np.unique(node[hit]))))


if __name__ == "__main__":
    main()

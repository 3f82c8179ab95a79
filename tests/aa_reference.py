"""The edge test of adaptive anti-aliasing, restated in typed numpy: rt/renderer.d:154-177 with tooDifferent
(rt/color.d:18-23), as include/c2rt.h specifies it for c2rt_render_frame_adaptive.  fp32 at every step, no library code.

    neighs  = {p(x, y), p(x > 0 ? x - 1 : x, y), p(x + 1 < W ? x + 1 : x, y), p(x, y > 0 ? y - 1 : y), p(x, y + 1 < H ? y + 1 : y)}
    average = ((((0 + n0) + n1) + n2) + n3) + n4, then / 5.0f, per channel
    flag    = any over i and channel of fabsf(neighs[i] - average) > threshold

Every intermediate is a numpy float32 array, so each operation rounds to fp32 once, as the C statement does without
contraction.  A NaN difference compares false.
"""
import numpy as np

TILE = 8    # the refinement kernel's tile: one wavefront, 8x8 pixels


def needs_aa(image, threshold=0.1):
    """(H, W) uint8 flags of an (H, W, 3) float32 image"""
    img = np.asarray(image)
    assert img.dtype == np.float32 and img.ndim == 3 and img.shape[2] == 3, (img.dtype, img.shape)
    thr = np.float32(threshold)
    h, w, _ = img.shape
    xs, ys = np.arange(w), np.arange(h)
    neighs = [img,
              img[:, np.maximum(xs - 1, 0)],
              img[:, np.minimum(xs + 1, w - 1)],
              img[np.maximum(ys - 1, 0)],
              img[np.minimum(ys + 1, h - 1)]]
    average = np.zeros_like(img)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in neighs:
            average = average + n
            assert average.dtype == np.float32
        average = average / np.float32(5.0)
        assert average.dtype == np.float32
        flag = np.zeros((h, w), dtype=bool)
        for n in neighs:
            diff = np.abs(n - average)
            assert diff.dtype == np.float32
            flag |= (diff > thr).any(axis=2)
    return flag.astype(np.uint8)


def tile_counts(mask):
    """flagged pixels of every 8x8 tile of an (H, W) mask, row-major over the tiles (partial tiles at the edges included)"""
    h, w = mask.shape
    return np.array([int(mask[y:y + TILE, x:x + TILE].sum()) for y in range(0, h, TILE) for x in range(0, w, TILE)])

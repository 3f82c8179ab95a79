"""Shared by tests/test_hit_layers_abi.py (CPU) and tests/test_gpu_hit_layers.py (GPU): the definition of the hit layers
(include/c2rt.h, "hit layers") over ANY single-hit trace, in numpy float64, and the cases both files use.

    o = ray.orig; d = ray.dir (never changed); total = 0.0
    for k in 0 .. K-1:
        rec = trace(o, d)
        if rec is a hit: rec.dist = rec.dist + total; total = rec.dist
        slot k := rec
        if rec is a miss: break
        o = rec.p + d * 1e-6
    count = number of hit records stored

numpy evaluates `p + d * 1e-6` as a product, rounded, then a sum, rounded: no contraction."""
import functools

import numpy as np

from chess2rt_amd.api import RAY_HIT_DTYPE

FIELDS = ("closest_node", "leaf_geom", "dist", "u", "v", "p", "normal")


def walk_layers(trace, rays, K, with_rgb=False):
    """The definition over `trace(rays (m, 6)) -> records` (any dtype with c2rt_ray_hit's field names; with_rgb:
    `-> (records, rgb (m, 3))`).  Returns (records [K][n] of RAY_HIT_DTYPE, count (n,) uint8[, rgb [K][n][3] float32]).
    Slots the rule leaves unwritten are zero here and have to be masked in comparisons: see `written`."""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = len(rays)
    recs = np.zeros((K, n), dtype=RAY_HIT_DTYPE)
    rgb = np.zeros((K, n, 3), dtype=np.float32)
    count = np.zeros(n, dtype=np.uint8)
    o, d = rays[:, :3].copy(), rays[:, 3:]
    total = np.zeros(n, dtype=np.float64)
    walking = np.arange(n)
    for k in range(K):
        if walking.size == 0:
            break
        got = trace(np.ascontiguousarray(np.hstack([o[walking], d[walking]])))
        if with_rgb:
            got, colour = got
            rgb[k, walking] = colour
        hit = np.asarray(got["closest_node"]) >= 0
        for f in FIELDS:
            recs[f][k, walking] = got[f]
        w_hit = walking[hit]
        with np.errstate(all="ignore"):
            dist = np.asarray(got["dist"], dtype=np.float64)[hit] + total[w_hit]       # one addition
            recs["dist"][k, w_hit] = dist
            total[w_hit] = dist
            count[w_hit] += 1
            step = d[w_hit] * 1e-6                                                      # the product ...
            o[w_hit] = np.asarray(got["p"], dtype=np.float64)[hit] + step               # ... then the sum
        walking = w_hit
    return (recs, count, rgb) if with_rgb else (recs, count)


def written(count, K):
    """[K][n] bool: slot k of ray i is written if and only if k <= count[i] (and k < K)"""
    return np.arange(K)[:, None] <= np.asarray(count, dtype=np.int64)[None, :]


def layer_rays(rays, recs, count, k):
    """(indices, rays) of layer k's stepped rays: the rays whose slot k is written — origin = layer k - 1's p + d * 1e-6"""
    rays = np.asarray(rays, dtype=np.float64)
    if k == 0:
        return np.arange(len(rays)), rays
    idx = np.nonzero(np.asarray(count) >= k)[0]
    with np.errstate(all="ignore"):
        o = recs["p"][k - 1, idx] + rays[idx, 3:] * 1e-6
    return idx, np.ascontiguousarray(np.hstack([o, rays[idx, 3:]]))


def bits_equal_where_written(got, want, mask):
    """every byte of the masked slots equal (structured records or plain arrays whose leading axes are the mask's)"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (g.shape, w.shape, g.dtype, w.dtype)
    gb = g.view(np.uint8).reshape(mask.shape + (-1,))
    wb = w.view(np.uint8).reshape(mask.shape + (-1,))
    return bool(np.array_equal(gb[mask], wb[mask]))


# ---- the cases of the GPU tests, with their oracle walks (computed once per process, read-only) ------------------------

LAYERS = 8          # max_layers of the GPU tests' full runs: no ray of any case has that many surfaces
TRUNCATED = 3
FRAME_LAYERS = 6
FRAME_SCENES = ("lecture5.sdl", "csg_stress.sdl")
# the cases whose preconditions the issue states (test_hit_layers_abi.py asserts them on the oracle alone)
EYELESS_RICH = ("lecture5", "csg_stress", "fuzz_depth0", "fuzz_depth1", "fuzz_depth2", "fuzz_depth3", "fuzz_depth4")


@functools.lru_cache(maxsize=None)
def eyeless_layers(name):
    """(scene, rays, oracle records [LAYERS][n], oracle count) of one scene of test_gpu_ray_queries.EYELESS"""
    from ray_query_util import oracle_trace
    from test_gpu_ray_queries import eyeless_case

    scene, rays, _ = eyeless_case(name)
    recs, count = walk_layers(lambda r: oracle_trace(scene.desc, r), rays, LAYERS)
    return scene, rays, recs, count


@functools.lru_cache(maxsize=None)
def frame_layers(scene_file):
    """(scene, cam, opts, screen rays, oracle records [LAYERS][W * H], oracle count) of test_gpu_ray_queries.frame_case"""
    from ray_query_util import oracle_trace
    from test_gpu_ray_queries import frame_case

    scene, cam, opts, rays, _ = frame_case(scene_file)
    recs, count = walk_layers(lambda r: oracle_trace(scene.desc, r), rays, LAYERS)
    return scene, cam, opts, rays, recs, count


def check_layer_preconditions(what, count):
    """the issue's bounds, on the oracle alone: depth to see, no truncation at LAYERS, truncation at TRUNCATED"""
    count = np.asarray(count, dtype=np.int64)
    deep, most = int((count >= 3).sum()), int(count.max())
    assert deep >= 100, (what, "rays with three or more layers", deep)
    assert most < LAYERS, (what, "a ray reaches max_layers", most)
    assert int((count >= TRUNCATED).sum()) >= 100, (what, "rays that max_layers = 3 truncates or ends exactly")
    return deep, most

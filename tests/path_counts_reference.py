"""The count rule of c2rt_path_counts, restated in numpy from the contract in include/c2rt.h: the reprojection and the
gather are tests/temporal_reference.py's, an array operation at a time in the contract's order, and the rule follows them,
so that counts, variance and age are the library's bit for bit.  Shared by tests/test_paths_counted_abi.py (CPU) and
tests/test_gpu_paths_counted.py (GPU).

Besides the planes it counts, into `classes`, the pixels by what became of them
  miss        node < 0
  no_history  a hit with no history given, or whose reprojection keeps no tap
  young       taps kept, the youngest below min_age
  at_max      old enough, counts == max_paths
  at_min      old enough, counts == min_paths (and below max_paths)
  between     old enough, min_paths < counts < max_paths
"""
import numpy as np

import temporal_reference as tr

CLASSES = ("miss", "no_history", "young", "at_min", "between", "at_max")
F0, F1 = np.float32(0.0), np.float32(1.0)


def path_counts(node, normal, p, channels, min_normal_dot, max_plane_dist, min_paths, max_paths, young_paths, min_age, paths_per_variance,
                prev_paths, prev_cam=None, history=None, prev_counts=None, classes=None):
    """c2rt_path_counts for full-frame guides node (H, W), normal and p (H, W, 3) float64; `history`: the previous
    history blob of `channels` channels (None: the first frame), `prev_cam` its camera, `prev_counts` (H, W) uint8 or
    None.  Returns dict(counts=(H, W) uint8, variance=(H, W) float32, age=(H, W) uint32)."""
    node = np.ascontiguousarray(node, dtype=np.int32)
    H, W = node.shape
    if classes is not None:
        for k in CLASSES:
            classes.setdefault(k, 0)
    hit = node >= 0
    counts = np.where(hit, young_paths, 0).astype(np.uint32)
    var = np.zeros((H, W), dtype=np.float32)
    age = np.zeros((H, W), dtype=np.uint32)
    have = np.zeros((H, W), dtype=bool)
    old = np.zeros((H, W), dtype=bool)
    if history is not None:
        with np.errstate(all="ignore"):
            normal = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
            p = np.asarray(p, dtype=np.float64).reshape(H, W, 3)
            nf, pf = normal.astype(np.float32), p.astype(np.float32)
            hs = tr.split_history(history, H, W, channels)
            given = np.full((H, W), prev_paths, dtype=np.uint32) if prev_counts is None else np.ascontiguousarray(prev_counts, dtype=np.uint8).astype(np.uint32)
            pos, na, nb, nc, det, Wd, Hd = tr.camera_constants(prev_cam, W, H)
            r = p - pos
            ka, kb, kc = tr._dot3(r, na), tr._dot3(r, nb), tr._dot3(r, nc)
            s = ka if det > 0 else -ka
            front = hit & (s > 0)
            sx, sy = (kb / ka) * Wd, (kc / ka) * Hd
            inframe = front & (sx > -1.0) & (sx < Wd) & (sy > -1.0) & (sy < Hd)
            sx, sy = np.where(inframe, sx, 0.0), np.where(inframe, sy, 0.0)
            x0d, y0d = np.floor(sx), np.floor(sy)
            fx, fy = (sx - x0d).astype(np.float32), (sy - y0d).astype(np.float32)
            x0, y0 = x0d.astype(np.int64), y0d.astype(np.int64)
            wx, wy = (F1 - fx, fx), (F1 - fy, fy)
            sumw = np.zeros((H, W), dtype=np.float32)
            s1, s2 = np.zeros((H, W), dtype=np.float32), np.zeros((H, W), dtype=np.float32)
            amin = np.full((H, W), 0xFFFFFFFF, dtype=np.uint32)
            cprev = np.zeros((H, W), dtype=np.uint32)
            for j in range(2):
                for i in range(2):
                    tx, ty = x0 + i, y0 + j
                    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                    xt, yt = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                    w = wx[i] * wy[j]
                    dn = tr._dot3f(nf, hs["nf"][yt, xt])
                    dp = tr._dot3f(nf, hs["pf"][yt, xt] - pf)
                    keep = (inframe & inside & (w > 0) & (hs["node"][yt, xt] == node) & (dn > np.float32(min_normal_dot))
                            & (np.abs(dp) <= np.float32(max_plane_dist)))
                    sumw = np.where(keep, sumw + w, sumw)
                    s1 = np.where(keep, s1 + w * hs["m"][yt, xt, 0], s1)
                    s2 = np.where(keep, s2 + w * hs["m"][yt, xt, 1], s2)
                    amin = np.where(keep, np.minimum(amin, hs["age"][yt, xt]), amin)
                    cprev = np.where(keep, np.maximum(cprev, given[yt, xt]), cprev)
            have = inframe & (sumw > 0)
            old = have & ~(amin < np.uint32(min_age))
            cprev = np.where(cprev == 0, 1, cprev).astype(np.uint32)
            m1, m2 = s1 / sumw, s2 / sumw
            v = m2 - m1 * m1
            v = np.where(v <= 0, F0, v).astype(np.float32)                   # a NaN stays
            t = (v * cprev.astype(np.float32)) * np.float32(paths_per_variance)
            below = t < np.float32(max_paths)
            tt = np.where(below & old, t, F0)
            k = tt.astype(np.uint32)
            k = np.where(k.astype(np.float32) < tt, k + 1, k).astype(np.uint32)
            k = np.maximum(k, np.uint32(min_paths))
            k = np.where(below, k, np.uint32(max_paths))
            counts = np.where(old, k, counts).astype(np.uint32)
            var = np.where(old, v, var).astype(np.float32)
            age = np.where(have, amin, age).astype(np.uint32)
            if classes is not None:
                top = old & (k == max_paths)
                classes["at_max"] += int(top.sum())
                classes["at_min"] += int((old & ~top & (k == min_paths)).sum())
                classes["between"] += int((old & (k > min_paths) & (k < max_paths)).sum())
    if classes is not None:
        classes["miss"] += int((~hit).sum())
        classes["no_history"] += int((hit & ~have).sum())
        classes["young"] += int((have & ~old).sum())
    return dict(counts=counts.astype(np.uint8), variance=np.ascontiguousarray(var), age=np.ascontiguousarray(age))

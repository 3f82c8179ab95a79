"""c2rt_temporal_accumulate_motion restated in numpy from the contract in include/c2rt.h, an array operation at a time in
the contract's order, so that planes and history are the library's bit for bit.  Pixels whose node is not listed are
temporal_reference.accumulate's own (that function is called, not copied); a pixel on a listed node is carried through
the node's record — composed here from the two poses as the host composes it — and runs the chain on the carried point
with the two squared tap tests.  Shared by tests/test_temporal_motion_abi.py (CPU) and tests/test_gpu_temporal_motion.py.

Into `counts` go temporal_reference's classes for the static pass and, for the pixels of the call itself,
  unlisted_history   a hit pixel on no listed node that found its history (its age is above 1: for max_age above 1)
  unlisted_restart   ... that did not
  moved_kept         a pixel on a listed node with at least one tap kept
  moved_rejected     ... reprojected into the frame, every tap dropped
  moved_lost         ... behind the previous camera, outside its frame, or a NaN chain
"""
import numpy as np

import temporal_reference as tr
from temporal_reference import F0, F1, _dot3, _dot3f

MOTION_CLASSES = ("unlisted_history", "unlisted_restart", "moved_kept", "moved_rejected", "moved_lost")
MAX_MOTION_NODES = 16


def compose(prev, cur):
    """the contract's "per moved node, on the host": (R, N, off_cur, off_prev) in fp64 from two transforms of 30 doubles"""
    prev, cur = (np.asarray(t, dtype=np.float64).reshape(30) for t in (prev, cur))
    Tc, Ic, oc = cur[0:9].reshape(3, 3), cur[9:18].reshape(3, 3), cur[27:30].copy()
    Tp, TIp, op = prev[0:9].reshape(3, 3), prev[18:27].reshape(3, 3), prev[27:30].copy()
    R, N = np.empty((3, 3), dtype=np.float64), np.empty((3, 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                R[i, j] = (Ic[i, 0] * Tp[0, j] + Ic[i, 1] * Tp[1, j]) + Ic[i, 2] * Tp[2, j]
                N[i, j] = (Tc[0, i] * TIp[0, j] + Tc[1, i] * TIp[1, j]) + Tc[2, i] * TIp[2, j]
    return R, N, oc, op


def carry(p, normal, record):
    """(p', n') of points and normals (..., 3) float64 through a record of compose()"""
    R, N, oc, op = record
    p, normal = np.asarray(p, dtype=np.float64), np.asarray(normal, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = p - oc
        pp = np.stack([((e[..., 0] * R[0, j] + e[..., 1] * R[1, j]) + e[..., 2] * R[2, j]) + op[j] for j in range(3)], axis=-1)
        nn = np.stack([(normal[..., 0] * N[0, j] + normal[..., 1] * N[1, j]) + normal[..., 2] * N[2, j] for j in range(3)], axis=-1)
    return pp, nn


def accumulate(node, normal, p, image, max_age, min_normal_dot, max_plane_dist, prev_cam=None, history=None, motion=None, counts=None):
    """c2rt_temporal_accumulate_motion; the arguments of temporal_reference.accumulate and `motion` = {node index: (prev,
    cur)} (None or empty: the static call).  Returns its dict."""
    static_counts = {} if counts is not None else None
    base = tr.accumulate(node, normal, p, image, max_age, min_normal_dot, max_plane_dist, prev_cam=prev_cam, history=history, counts=static_counts)
    node = np.ascontiguousarray(node, dtype=np.int32)
    H, W = node.shape
    motion = dict(motion or {})
    assert len(motion) <= MAX_MOTION_NODES
    IN = np.ascontiguousarray(image, dtype=np.float32).reshape(H, W, -1)
    CH = IN.shape[2]
    hit = node >= 0
    moved = np.zeros((H, W), dtype=bool)
    for index in motion:
        moved |= hit & (node == np.int64(index))
    if counts is not None:
        for k in MOTION_CLASSES:
            counts.setdefault(k, 0)
        for k, v in static_counts.items():
            counts[k] = counts.get(k, 0) + v
    if history is None or not moved.any():
        if counts is not None and history is not None:
            have0 = np.asarray(base["age"]) > 1
            counts["unlisted_history"] += int((hit & have0).sum())
            counts["unlisted_restart"] += int((hit & ~have0).sum())
        return base
    with np.errstate(all="ignore"):
        normal = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
        p = np.asarray(p, dtype=np.float64).reshape(H, W, 3)
        pc, nc = p.copy(), normal.copy()
        for index, (prev, cur) in motion.items():
            mask = hit & (node == np.int64(index))
            pp, nn = carry(p, normal, compose(prev, cur))
            pc[mask], nc[mask] = pp[mask], nn[mask]
        nf, pf = nc.astype(np.float32), pc.astype(np.float32)
        l2 = (nf[..., 0] * nf[..., 0] + nf[..., 1] * nf[..., 1]) + nf[..., 2] * nf[..., 2]
        mn2 = np.float32(min_normal_dot) * np.float32(min_normal_dot)
        mp2 = np.float32(max_plane_dist) * np.float32(max_plane_dist)
        lum = tr.luminance(IN)
        lum2 = lum * lum
        hs = tr.split_history(history, H, W, CH)
        pos, na, nb, ncam, det, Wd, Hd = tr.camera_constants(prev_cam, W, H)
        r = pc - pos
        ka, kb, kc = _dot3(r, na), _dot3(r, nb), _dot3(r, ncam)
        s = ka if det > 0 else -ka
        front = moved & (s > 0)
        sx, sy = (kb / ka) * Wd, (kc / ka) * Hd
        inframe = front & (sx > -1.0) & (sx < Wd) & (sy > -1.0) & (sy < Hd)
        sx, sy = np.where(inframe, sx, 0.0), np.where(inframe, sy, 0.0)
        x0d, y0d = np.floor(sx), np.floor(sy)
        fx, fy = (sx - x0d).astype(np.float32), (sy - y0d).astype(np.float32)
        x0, y0 = x0d.astype(np.int64), y0d.astype(np.int64)
        wx, wy = (F1 - fx, fx), (F1 - fy, fy)
        sumw = np.zeros((H, W), dtype=np.float32)
        total = np.zeros((H, W, CH), dtype=np.float32)
        s1, s2 = np.zeros((H, W), dtype=np.float32), np.zeros((H, W), dtype=np.float32)
        amin = np.full((H, W), 0xFFFFFFFF, dtype=np.uint32)
        for j in range(2):
            for i in range(2):
                tx, ty = x0 + i, y0 + j
                inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                xt, yt = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                w = wx[i] * wy[j]
                positive = w > 0
                same = hs["node"][yt, xt] == node
                dn = _dot3f(nf, hs["nf"][yt, xt])
                facing = (dn > 0) & (dn * dn > mn2 * l2)
                dp = _dot3f(nf, hs["pf"][yt, xt] - pf)
                near = dp * dp <= mp2 * l2
                keep = inframe & inside & positive & same & facing & near
                sumw = np.where(keep, sumw + w, sumw)
                total = np.where(keep[..., None], total + w[..., None] * hs["c"][yt, xt], total)
                s1 = np.where(keep, s1 + w * hs["m"][yt, xt, 0], s1)
                s2 = np.where(keep, s2 + w * hs["m"][yt, xt, 1], s2)
                amin = np.where(keep, np.minimum(amin, hs["age"][yt, xt]), amin)
        have = inframe & (sumw > 0)
        h = total / sumw[..., None]
        m1, m2 = s1 / sumw, s2 / sumw
        cnt = np.minimum(amin.astype(np.uint64) + 1, np.uint64(max_age)).astype(np.uint32)
        a = F1 / cnt.astype(np.float32)
        colour_h = h + (IN - h) * a[..., None]
        M1h = m1 + (lum - m1) * a
        M2h = m2 + (lum2 - m2) * a
        v = M2h - M1h * M1h
        var_h = np.where(v > 0, v, F0)
        # a moved pixel: its history, or a restart
        colour_m = np.where(have[..., None], colour_h, IN)
        M1m, M2m = np.where(have, M1h, lum), np.where(have, M2h, lum2)
        var_m = np.where(have, var_h, F0)
        age_m = np.where(have, cnt, 1).astype(np.uint32)
    bh = tr.split_history(base["history"], H, W, CH)
    colour = np.where(moved[..., None], colour_m, base["colour"].reshape(H, W, CH)).astype(np.float32)
    M = np.where(moved[..., None], np.stack([M1m, M2m], axis=-1), bh["m"]).astype(np.float32)
    var = np.where(moved, var_m, base["variance"]).astype(np.float32)
    age = np.where(moved, age_m, base["age"]).astype(np.uint32)
    if counts is not None:
        have0 = np.asarray(base["age"]) > 1
        counts["unlisted_history"] += int((hit & ~moved & have0).sum())
        counts["unlisted_restart"] += int((hit & ~moved & ~have0).sum())
        counts["moved_kept"] += int(have.sum())
        counts["moved_rejected"] += int((inframe & ~have).sum())
        counts["moved_lost"] += int((moved & ~inframe).sum())
    out_hist = tr.join_history(bh["nf"], node, bh["pf"], age, colour, M)   # the CURRENT nf, pf: what the static pass wrote
    return dict(colour=np.ascontiguousarray(colour).reshape(base["colour"].shape), variance=np.ascontiguousarray(var), age=age, history=out_hist)


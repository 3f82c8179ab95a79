"""The temporal accumulation of c2rt_temporal_accumulate, restated in numpy from the contract in include/c2rt.h: the
reprojection an fp64 array operation at a time, the gather an fp32 array operation at a time, in the contract's order
(numpy does not contract a multiply and an add), so that planes and history are the library's bit for bit.  Shared by
tests/test_temporal_abi.py (CPU) and tests/test_gpu_temporal.py (GPU).

Besides the planes it counts, into `counts`, the pixels by what became of them
  miss        node < 0
  first       a hit, and no history was given
  behind      a hit whose point is not in front of the previous camera (!(s > 0))
  outside     reprojected outside the frame
  disoccluded reprojected into the frame, no tap kept
  partial     one to three taps kept
  full        all four taps kept
and, of the four taps of every pixel reprojected into the frame, the taps by the first test that drops them
  tap_outside the tap is outside the frame
  tap_zero    !(w > 0): a bilinear weight of zero, NaN, or underflow
  tap_other   the history's node there is another one
  tap_normal  !(dn > min_normal_dot)
  tap_plane   !(|dp| <= max_plane_dist)
  tap_kept
"""
import numpy as np

PIXEL_CLASSES = ("miss", "first", "behind", "outside", "disoccluded", "partial", "full")
TAP_CLASSES = ("tap_outside", "tap_zero", "tap_other", "tap_normal", "tap_plane", "tap_kept")
MAX_AGE = 65535
F0, F1 = np.float32(0.0), np.float32(1.0)
LR, LG, LB = np.float32(0.2126), np.float32(0.7152), np.float32(0.0722)


def history_bytes(width, height, channels):
    return width * height * (32 + 4 * channels + 8)


def split_history(blob, height, width, channels):
    """the planar history as arrays (views of `blob`): nf, pf (H, W, 3) float32, node (H, W) int32, age (H, W) uint32,
    c (H, W, channels) float32, m (H, W, 2) float32"""
    blob = np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
    px = width * height
    assert blob.size == history_bytes(width, height, channels), (blob.size, width, height, channels)
    g0 = blob[:16 * px].view(np.float32).reshape(height, width, 4)
    g1 = blob[16 * px:32 * px].view(np.float32).reshape(height, width, 4)
    c = blob[32 * px:(32 + 4 * channels) * px].view(np.float32).reshape(height, width, channels)
    m = blob[(32 + 4 * channels) * px:].view(np.float32).reshape(height, width, 2)
    return dict(nf=g0[..., :3], node=g0[..., 3].view(np.int32), pf=g1[..., :3], age=g1[..., 3].view(np.uint32), c=c, m=m)


def join_history(nf, node, pf, age, c, m):
    """the blob of those arrays (a new uint8 array)"""
    h, w = np.asarray(node).shape
    g0 = np.empty((h, w, 4), dtype=np.float32)
    g0[..., :3] = nf
    g0[..., 3] = np.ascontiguousarray(node, dtype=np.int32).view(np.float32)
    g1 = np.empty((h, w, 4), dtype=np.float32)
    g1[..., :3] = pf
    g1[..., 3] = np.ascontiguousarray(age, dtype=np.uint32).view(np.float32)
    parts = [g0, g1, np.ascontiguousarray(c, dtype=np.float32).reshape(h, w, -1), np.ascontiguousarray(m, dtype=np.float32).reshape(h, w, 2)]
    return np.concatenate([x.reshape(-1).view(np.uint8) for x in parts])


def _v3(cam, name):
    v = cam[name] if isinstance(cam, dict) else getattr(cam, name)
    return np.array([float(v[k]) for k in range(3)], dtype=np.float64)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=np.float64)


def camera_constants(cam, width, height):
    """the contract's "per call, on the host": (pos, na, nb, nc, det, Wd, Hd) in fp64; `cam`: a c2rt_camera_frame, or a
    dict of pos, up_left, up_right, down_left"""
    pos, ul, ur, dl = (_v3(cam, k) for k in ("pos", "up_left", "up_right", "down_left"))
    A, U, V = ul - pos, ur - ul, dl - ul
    na, nb, nc = _cross(U, V), _cross(V, A), _cross(A, U)
    det = (A[0] * na[0] + A[1] * na[1]) + A[2] * na[2]
    return pos, na, nb, nc, det, np.float64(width), np.float64(height)


def _dot3(a, b):
    return (a[..., 0] * b[0] + a[..., 1] * b[1]) + a[..., 2] * b[2]


def _dot3f(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def luminance(image):
    """(H, W, channels) float32 -> (H, W) float32"""
    if image.shape[2] == 1:
        return image[..., 0]
    return (LR * image[..., 0] + LG * image[..., 1]) + LB * image[..., 2]


def accumulate(node, normal, p, image, max_age, min_normal_dot, max_plane_dist, prev_cam=None, history=None, counts=None):
    """c2rt_temporal_accumulate for full-frame guides node (H, W), normal and p (H, W, 3) float64 and `image` (H, W,
    channels) or (H, W) float32; `history`: the previous history blob (None: the first frame), `prev_cam` its camera.
    Returns dict(colour=float32 of `image`'s shape, variance=(H, W) float32, age=(H, W) uint32, history=uint8 blob)."""
    node = np.ascontiguousarray(node, dtype=np.int32)
    image = np.ascontiguousarray(image, dtype=np.float32)
    shape = image.shape
    H, W = node.shape
    IN = image.reshape(H, W, -1)
    CH = IN.shape[2]
    if counts is not None:
        for k in PIXEL_CLASSES + TAP_CLASSES:
            counts.setdefault(k, 0)
    with np.errstate(all="ignore"):
        normal = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
        p = np.asarray(p, dtype=np.float64).reshape(H, W, 3)
        nf, pf = normal.astype(np.float32), p.astype(np.float32)
        hit = node >= 0
        lum = luminance(IN)
        lum2 = lum * lum
        have = np.zeros((H, W), dtype=bool)
        if history is not None:
            hs = split_history(history, H, W, CH)
            pos, na, nb, nc, det, Wd, Hd = camera_constants(prev_cam, W, H)
            r = p - pos
            ka, kb, kc = _dot3(r, na), _dot3(r, nb), _dot3(r, nc)
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
            total = np.zeros((H, W, CH), dtype=np.float32)
            s1, s2 = np.zeros((H, W), dtype=np.float32), np.zeros((H, W), dtype=np.float32)
            amin = np.full((H, W), 0xFFFFFFFF, dtype=np.uint32)
            nkept = np.zeros((H, W), dtype=np.int64)
            for j in range(2):
                for i in range(2):
                    tx, ty = x0 + i, y0 + j
                    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                    xt, yt = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                    w = wx[i] * wy[j]
                    positive = w > 0
                    same = hs["node"][yt, xt] == node
                    dn = _dot3f(nf, hs["nf"][yt, xt])
                    facing = dn > np.float32(min_normal_dot)
                    dp = _dot3f(nf, hs["pf"][yt, xt] - pf)
                    near = np.abs(dp) <= np.float32(max_plane_dist)
                    keep = inframe & inside & positive & same & facing & near
                    sumw = np.where(keep, sumw + w, sumw)
                    total = np.where(keep[..., None], total + w[..., None] * hs["c"][yt, xt], total)
                    s1 = np.where(keep, s1 + w * hs["m"][yt, xt, 0], s1)
                    s2 = np.where(keep, s2 + w * hs["m"][yt, xt, 1], s2)
                    amin = np.where(keep, np.minimum(amin, hs["age"][yt, xt]), amin)
                    nkept += keep
                    if counts is not None:
                        left = inframe
                        for name, ok in (("tap_outside", inside), ("tap_zero", positive), ("tap_other", same), ("tap_normal", facing), ("tap_plane", near)):
                            counts[name] += int((left & ~ok).sum())
                            left = left & ok
                        counts["tap_kept"] += int(left.sum())
            have = inframe & (sumw > 0)
            if counts is not None:
                counts["behind"] += int((hit & ~front).sum())
                counts["outside"] += int((front & ~inframe).sum())
                counts["disoccluded"] += int((inframe & ~have).sum())
                counts["partial"] += int((have & (nkept < 4)).sum())
                counts["full"] += int((have & (nkept == 4)).sum())
            h = total / sumw[..., None]
            m1, m2 = s1 / sumw, s2 / sumw
            cnt = np.minimum(amin.astype(np.uint64) + 1, np.uint64(max_age)).astype(np.uint32)
            a = F1 / cnt.astype(np.float32)
            colour_h = h + (IN - h) * a[..., None]
            M1h = m1 + (lum - m1) * a
            M2h = m2 + (lum2 - m2) * a
            v = M2h - M1h * M1h
            var_h = np.where(v > 0, v, F0)
        elif counts is not None:
            counts["first"] += int(hit.sum())
        if counts is not None:
            counts["miss"] += int((~hit).sum())
        colour = IN.copy()
        M1 = np.where(hit, lum, F0)
        M2 = np.where(hit, lum2, F0)
        var = np.zeros((H, W), dtype=np.float32)
        age = np.where(hit, 1, 0).astype(np.uint32)
        if history is not None:
            colour = np.where(have[..., None], colour_h, colour)
            M1, M2 = np.where(have, M1h, M1), np.where(have, M2h, M2)
            var = np.where(have, var_h, var)
            age = np.where(have, cnt, age).astype(np.uint32)
    colour = np.ascontiguousarray(colour, dtype=np.float32)
    out_hist = join_history(nf, node, pf, age, colour, np.stack([M1, M2], axis=-1).astype(np.float32))
    return dict(colour=colour.reshape(shape), variance=np.ascontiguousarray(var, dtype=np.float32), age=age, history=out_hist)


def count_differing(a, b):
    """float32 values that differ, a NaN equal to any NaN: the contract fixes which values are NaN, not a NaN's sign and
    payload"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))).sum())


def history_differing(a, b, height, width, channels):
    """values of two history blobs that differ: node and age as integers, the rest as floats with count_differing's rule"""
    x, y = split_history(a, height, width, channels), split_history(b, height, width, channels)
    n = int((x["node"] != y["node"]).sum()) + int((x["age"] != y["age"]).sum())
    return n + sum(count_differing(x[k], y[k]) for k in ("nf", "pf", "c", "m"))

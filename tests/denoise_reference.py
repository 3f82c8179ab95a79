"""The a-trous filter of c2rt_denoise, restated in numpy from the contract in include/c2rt.h: every operation an fp32
array operation in the contract's order (numpy does not contract a multiply and an add), so that the result is the
library's bit for bit.  Shared by tests/test_denoise_abi.py (CPU) and tests/test_gpu_denoise.py (GPU).

Besides the image it counts the taps by what became of them, so that a test can show that a comparison exercises every
branch: of the 24 taps around every HIT pixel at every level
  outside   the tap is outside the frame
  other     it lies on another node (or on none)
  normal    same node, but !(dn > 0)
  dropped   same node, dn > 0, but !(w > 0): NaN, or underflow to zero
  soft      kept, with w below half its kernel weight K[i] * K[j]: an edge-stopping term is at work
  kept      kept, the rest
"""
import numpy as np

K = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16], dtype=np.float32)
CLASSES = ("outside", "other", "normal", "dropped", "soft", "kept")
F1 = np.float32(1.0)


def factors(levels, sigma_plane, sigma_colour):
    """(inv_plane, [inv_c2 of level 0 .. levels-1]) in fp32, as the contract computes them per call and per level"""
    with np.errstate(all="ignore"):
        inv_plane = F1 / np.float32(sigma_plane)
        inv_c2 = []
        for l in range(levels):
            sc = np.float32(sigma_colour) * np.float32(2.0 ** -l)
            inv_c2.append(F1 / (sc * sc))
    return inv_plane, inv_c2


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _level(node, nf, pf, C, s, power, inv_plane, inv_c2, colour, counts):
    H, W = node.shape
    hit = node >= 0
    sumw = np.zeros((H, W), dtype=np.float32)
    total = np.zeros_like(C)
    for j in range(-2, 3):
        ys = np.arange(H) + j * s
        for i in range(-2, 3):
            xs = np.arange(W) + i * s
            if i == 0 and j == 0:
                w = np.full((H, W), K[2] * K[2], dtype=np.float32)
                keep, Ct = hit, C
            else:
                inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
                yt, xt = np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]
                node_t, nf_t, pf_t, Ct = node[yt, xt], nf[yt, xt], pf[yt, xt], C[yt, xt]
                same = inside & (node_t == node)
                dn = _dot3(nf, nf_t)
                facing = dn > 0
                wn = dn
                for _ in range(power):
                    wn = wn * wn
                e = _dot3(nf, pf_t - pf) * inv_plane
                kij = K[i + 2] * K[j + 2]
                w = (kij * wn) * (F1 / (F1 + e * e))
                if colour:
                    dc = Ct - C
                    d2 = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2] if C.shape[2] == 3 else dc[..., 0] * dc[..., 0]
                    w = w * (F1 / (F1 + d2 * inv_c2))
                positive = w > 0
                keep = hit & same & facing & positive
                if counts is not None:
                    counts["outside"] += int((hit & ~inside).sum())
                    counts["other"] += int((hit & inside & ~same).sum())
                    counts["normal"] += int((hit & same & ~facing).sum())
                    counts["dropped"] += int((hit & same & facing & ~positive).sum())
                    soft = keep & (w < np.float32(0.5) * kij)
                    counts["soft"] += int(soft.sum())
                    counts["kept"] += int((keep & ~soft).sum())
            total = np.where(keep[..., None], total + w[..., None] * Ct, total)
            sumw = np.where(keep, sumw + w, sumw)
    return np.where(hit[..., None], total / sumw[..., None], C)


def denoise(node, normal, p, image, levels, normal_power_log2, sigma_plane, sigma_colour=0.0, albedo=None, base=None, counts=None):
    """c2rt_denoise for full-frame guides node (H, W), normal and p (H, W, 3) float64 and `image` (H, W, channels) or
    (H, W) float32; `counts`: a dict that takes the tap counts of CLASSES, summed over the levels.  Returns float32 of
    `image`'s shape."""
    node = np.asarray(node, dtype=np.int32)
    image = np.asarray(image, dtype=np.float32)
    shape = image.shape
    H, W = node.shape
    C = image.reshape(H, W, -1)
    if counts is not None:
        for k in CLASSES:
            counts.setdefault(k, 0)
    with np.errstate(all="ignore"):
        nf = np.asarray(normal, dtype=np.float64).reshape(H, W, 3).astype(np.float32)
        pf = np.asarray(p, dtype=np.float64).reshape(H, W, 3).astype(np.float32)
        inv_plane, inv_c2 = factors(levels, sigma_plane, sigma_colour)
        for l in range(levels):
            C = _level(node, nf, pf, C, 1 << l, int(normal_power_log2), inv_plane, inv_c2[l], float(sigma_colour) > 0, counts)
        if albedo is not None:
            C = np.asarray(albedo, dtype=np.float32).reshape(C.shape) * C
        if base is not None:
            C = np.asarray(base, dtype=np.float32).reshape(C.shape) + C
    return np.ascontiguousarray(C, dtype=np.float32).reshape(shape)


def same_bits(a, b):
    """bit for bit, except that a NaN equals any NaN: the contract fixes which values are NaN, not a NaN's sign and payload"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def count_differing(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))).sum())

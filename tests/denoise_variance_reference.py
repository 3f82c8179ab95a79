"""The variance-guided a-trous filter of c2rt_denoise_variance, restated in numpy from the contract in include/c2rt.h: every
operation an fp32 array operation in the contract's order (numpy does not contract a multiply and an add), so that the
result is the library's bit for bit.  Shared by tests/test_denoise_variance_abi.py (CPU) and
tests/test_gpu_denoise_variance.py (GPU).

Besides the two planes it counts, so that a test can show that a comparison exercises every branch:
  young, temporal   hit pixels of stage A that took the spatial estimate / kept their temporal variance
  per level (counts["levels"][l]) and summed over the levels:
  soft_lum          kept taps whose luminance factor 1 / (1 + dl^2 * inv_l) is below one half
  dropped_lum       taps whose weight was positive before the luminance factor and failed !(w > 0) after it
  kept              every kept tap (the centre not counted)
"""
import numpy as np

from denoise_reference import K, _dot3, count_differing, same_bits  # noqa: F401  (the last two re-exported for the tests)

F = np.float32
F0, F1 = F(0.0), F(1.0)
G = np.array([[1.0 / 16, 1.0 / 8, 1.0 / 16], [1.0 / 8, 1.0 / 4, 1.0 / 8], [1.0 / 16, 1.0 / 8, 1.0 / 16]], dtype=np.float32)
MAX_MIN_AGE = 64
COUNTS = ("young", "temporal", "soft_lum", "dropped_lum", "kept")


def lum(C):
    """(H, W, channels) -> (H, W)"""
    if C.shape[-1] == 3:
        return (F(0.2126) * C[..., 0] + F(0.7152) * C[..., 1]) + F(0.0722) * C[..., 2]
    return C[..., 0]


def _shifted(a, dy, dx):
    """(a[y + dy, x + dx] with the indices clipped, and the mask of the (y, x) whose neighbour lies inside the frame)"""
    H, W = a.shape[:2]
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    return a[np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]], inside


def _guide_weights(node, nf, pf, dy, dx, power, inv_plane):
    """the filter's tests and terms of the tap (dy, dx) pixels away: (same node and inside, dn > 0, wn, wp)"""
    node_t, inside = _shifted(node, dy, dx)
    nf_t, _ = _shifted(nf, dy, dx)
    pf_t, _ = _shifted(pf, dy, dx)
    same = inside & (node_t == node)
    dn = _dot3(nf, nf_t)
    wn = dn
    for _ in range(power):
        wn = wn * wn
    e = _dot3(nf, pf_t - pf) * inv_plane
    return same, dn > 0, wn, F1 / (F1 + e * e)


def estimate(node, nf, pf, C, variance, age, min_age, power, inv_plane, counts=None):
    """stage A: V0"""
    hit = node >= 0
    V0 = np.where(hit, variance, F0).astype(np.float32)
    young = hit & (age < min_age) if age is not None and min_age else np.zeros_like(hit)
    if counts is not None:
        counts["young"] += int(young.sum())
        counts["temporal"] += int((hit & ~young).sum())
    if not young.any():
        return V0
    L = lum(C)
    sumw, s1, s2 = (np.zeros(node.shape, dtype=np.float32) for _ in range(3))
    for j in range(-3, 4):
        for i in range(-3, 4):
            if i == 0 and j == 0:
                w, keep, l = np.ones(node.shape, dtype=np.float32), young, L
            else:
                same, facing, wn, wp = _guide_weights(node, nf, pf, j, i, power, inv_plane)
                w = wn * wp
                keep = young & same & facing & (w > 0)
                l, _ = _shifted(L, j, i)
            s1 = np.where(keep, s1 + w * l, s1)
            s2 = np.where(keep, s2 + w * (l * l), s2)
            sumw = np.where(keep, sumw + w, sumw)
    m1, m2 = s1 / sumw, s2 / sumw
    v = m2 - m1 * m1
    v = np.where(v > 0, v, F0)
    boost = F(min_age) / np.maximum(age, 1).astype(np.float32)
    return np.where(young, v * boost, V0).astype(np.float32)


def _level(node, nf, pf, C, V, s, power, inv_plane, sl2, var_floor, lum_on, counts):
    hit = node >= 0
    if lum_on:
        gs, gw = np.zeros(node.shape, dtype=np.float32), np.zeros(node.shape, dtype=np.float32)
        for j in range(-1, 2):
            for i in range(-1, 2):
                Vt, inside = _shifted(V, j, i)
                gs = np.where(inside, gs + G[j + 1, i + 1] * Vt, gs)
                gw = np.where(inside, gw + G[j + 1, i + 1], gw)
        g = gs / gw
        inv_l = F1 / (sl2 * g + var_floor)
        L = lum(C)
    sumw, sv = np.zeros(node.shape, dtype=np.float32), np.zeros(node.shape, dtype=np.float32)
    total = np.zeros_like(C)
    for j in range(-2, 3):
        for i in range(-2, 3):
            if i == 0 and j == 0:
                w, keep, Ct, Vt = np.full(node.shape, K[2] * K[2], dtype=np.float32), hit, C, V
            else:
                same, facing, wn, wp = _guide_weights(node, nf, pf, j * s, i * s, power, inv_plane)
                Ct, _ = _shifted(C, j * s, i * s)
                Vt, _ = _shifted(V, j * s, i * s)
                w = ((K[i + 2] * K[j + 2]) * wn) * wp
                before = w > 0
                if lum_on:
                    Lt, _ = _shifted(L, j * s, i * s)
                    dl = Lt - L
                    lf = F1 / (F1 + (dl * dl) * inv_l)
                    w = w * lf
                keep = hit & same & facing & (w > 0)
                if counts is not None:
                    counts["kept"] += int(keep.sum())
                    if lum_on:
                        counts["soft_lum"] += int((keep & (lf < F(0.5))).sum())
                        counts["dropped_lum"] += int((hit & same & facing & before & ~(w > 0)).sum())
            total = np.where(keep[..., None], total + w[..., None] * Ct, total)
            sumw = np.where(keep, sumw + w, sumw)
            sv = np.where(keep, sv + (w * w) * Vt, sv)
    return np.where(hit[..., None], total / sumw[..., None], C), np.where(hit, sv / (sumw * sumw), V)


def denoise_variance(node, normal, p, image, variance, age=None, levels=5, normal_power_log2=5, sigma_plane=1.0, sigma_lum=4.0, var_floor=1e-8,
                     min_age=4, albedo=None, base=None, counts=None):
    """c2rt_denoise_variance for full-frame guides node (H, W), normal and p (H, W, 3) float64, `image` (H, W, channels) or
    (H, W) float32, `variance` (H, W) float32 and `age` (H, W) uint32 or None; `counts`: a dict that takes COUNTS, summed, and
    under "levels" one dict per level.  Returns (out of `image`'s shape, variance_out (H, W)), float32."""
    node = np.asarray(node, dtype=np.int32)
    image = np.asarray(image, dtype=np.float32)
    shape = image.shape
    H, W = node.shape
    C = image.reshape(H, W, -1)
    V = np.asarray(variance, dtype=np.float32).reshape(H, W)
    if age is not None:
        age = np.asarray(age, dtype=np.uint32).reshape(H, W)
    if counts is not None:
        for k in COUNTS:
            counts.setdefault(k, 0)
        counts.setdefault("levels", [])
    with np.errstate(all="ignore"):
        nf = np.asarray(normal, dtype=np.float64).reshape(H, W, 3).astype(np.float32)
        pf = np.asarray(p, dtype=np.float64).reshape(H, W, 3).astype(np.float32)
        inv_plane = F1 / F(sigma_plane)
        sl2 = F(sigma_lum) * F(sigma_lum)
        V = estimate(node, nf, pf, C, V, age, int(min_age), int(normal_power_log2), inv_plane, counts)
        for l in range(levels):
            per = dict.fromkeys(COUNTS, 0) if counts is not None else None
            C, V = _level(node, nf, pf, C, V, 1 << l, int(normal_power_log2), inv_plane, sl2, F(var_floor), float(sigma_lum) > 0, per)
            if counts is not None:
                counts["levels"].append(per)
                for k in ("soft_lum", "dropped_lum", "kept"):
                    counts[k] += per[k]
        if albedo is not None:
            C = np.asarray(albedo, dtype=np.float32).reshape(C.shape) * C
        if base is not None:
            C = np.asarray(base, dtype=np.float32).reshape(C.shape) + C
    return np.ascontiguousarray(C, dtype=np.float32).reshape(shape), np.ascontiguousarray(V, dtype=np.float32)

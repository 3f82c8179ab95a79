"""A numpy restatement of the occlusion planes' definition (include/c2rt.h, "occlusion planes"), independent of the
library: no library code, only tests/camera_reference.py's restatements of the three build-defined routines the lens
samples already use (hash32 / rng_key, rng_uniform, lens_sincos2pi).

For sample index idx, record rec (what c2rt_trace_rays returns for the ray) and ray direction d:

    hit:   N    = dot(d, rec.normal) < 0 ? rec.normal : -rec.normal
           from = rec.p + N * 1e-6
           key  = rng_key(seed, idx, 0)
           for s in 0 .. K-1:
               u = rng_uniform(key, s, 0);  v = rng_uniform(key, s, 1)
               (sn, cs) = lens_sincos2pi(u)
               w = 2.0 * v - 1.0;  c = sqrt(1.0 - w * w)
               res = (cs * c, -w, sn * c);  if ((res.x*N.x + res.y*N.y) + res.z*N.z) < 0: res = -res
               to = from + res * radius
               if visible(from, to): open |= 1 << s; bent += res
           ao = float32(popcount(open)) / float32(K)
    miss:  open = low K bits, ao = 1.0f, bent = +0, +0, +0; no sample is drawn

Every operation is a numpy float64 +, * or sqrt (IEEE, never contracted), in the order written.  The visibility of a
segment is NOT decided here: `samples` returns the segments, the caller has them answered (by the library's visibility
query, or the oracle's) and hands the answers to `planes`.

Vectorised over the n samples of a call and their K draws."""
import numpy as np

import camera_reference as cr

F32, F64, U64 = np.float32, np.float64, np.uint64
MAX_SAMPLES = 64


def uniforms(seed, idx, K):
    """(u, v), each (n, K): draws 0 and 1 of sample s of the key of index idx"""
    idx = np.asarray(idx, dtype=U64).reshape(-1)
    key = cr.rng_key(int(seed), idx, 0)
    s = np.arange(K, dtype=np.uint32)
    return cr.rng_uniform(key[:, None], s[None, :], 0), cr.rng_uniform(key[:, None], s[None, :], 1)


def unflipped(u, v):
    """hemisphereSample's `res` before its flip, for arrays u, v of one shape: (..., 3)"""
    u, v = np.asarray(u, dtype=F64), np.asarray(v, dtype=F64)
    sn, cs = cr.lens_sincos2pi(u.reshape(-1))
    sn, cs = sn.reshape(u.shape), cs.reshape(u.shape)
    w = F64(2.0) * v - F64(1.0)
    c = np.sqrt(F64(1.0) - w * w)
    return np.stack([cs * c, -w, sn * c], axis=-1)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def flipped(res, N):
    """(res with the flip applied, which were flipped); N broadcasts against res"""
    with np.errstate(invalid="ignore"):
        flip = dot3(res, N) < 0
    return np.where(flip[..., None], -res, res), flip


def faceforward(d, n):
    with np.errstate(invalid="ignore", over="ignore"):
        front = dot3(d, n) < 0
    return np.where(front[..., None], n, -n)


def samples(records, dirs, idx, K, radius, seed):
    """records: RAY_HIT_DTYPE (n,), dirs (n, 3), idx (n,).  Returns (hit (n,) bool, res (n, K, 3), segments (n, K, 6),
    flip (n, K) bool); rows of misses are zeros: a miss draws nothing."""
    assert 1 <= K <= MAX_SAMPLES
    n = len(records)
    hit = records["closest_node"] >= 0
    res = np.zeros((n, K, 3), dtype=F64)
    seg = np.zeros((n, K, 6), dtype=F64)
    flip = np.zeros((n, K), dtype=bool)
    if hit.any():
        with np.errstate(invalid="ignore", over="ignore"):
            N = faceforward(np.asarray(dirs, dtype=F64)[hit], records["normal"][hit])
            frm = records["p"][hit] + N * F64(1e-6)
            u, v = uniforms(seed, np.asarray(idx)[hit], K)
            r, f = flipped(unflipped(u, v), N[:, None, :])
            to = frm[:, None, :] + r * F64(radius)
        res[hit], flip[hit] = r, f
        seg[hit] = np.concatenate([np.broadcast_to(frm[:, None, :], to.shape), to], axis=-1)
    return hit, res, seg, flip


def planes(records, res, visible, K):
    """The four planes from the directions of `samples` and the segments' answers `visible` (n, K) (rows of misses are
    not read): {node int32 (n,), open uint64 (n,), ao float32 (n,), bent float64 (n, 3)}"""
    n = len(records)
    hit = records["closest_node"] >= 0
    vis = (np.asarray(visible).reshape(n, K) != 0) & hit[:, None]
    low = U64((1 << K) - 1)
    opened = np.zeros(n, dtype=U64)
    bent = np.zeros((n, 3), dtype=F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(K):
            on = vis[:, s]
            opened[on] |= U64(1 << s)
            bent[on] = bent[on] + res[on, s]
    opened[~hit] = low
    count = np.array([bin(int(x)).count("1") for x in opened], dtype=np.int64)
    ao = count.astype(F32) / F32(K)
    return {"node": records["closest_node"].astype(np.int32), "open": opened, "ao": ao.astype(F32), "bent": bent}


def mask_kinds(opened, hit, K):
    """(mixed, full, empty) among the hits"""
    low = U64((1 << K) - 1)
    o = np.asarray(opened)[hit]
    return int(((o != 0) & (o != low)).sum()), int((o == low).sum()), int((o == 0).sum())

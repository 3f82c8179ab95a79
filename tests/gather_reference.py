"""A numpy restatement of the gather planes' definition (include/c2rt.h, "gather planes"), independent of the library.
The directions and origins are tests/occlusion_reference.py's (`samples`, at any radius: only `res` and `from` are used);
what is restated here is the weight, the fp32 sums, the division and the product, in the types of the definition:

    hit:   for s in 0 .. K-1:
               cosw = (res.x*N.x + res.y*N.y) + res.z*N.z          float64
               w    = float32(2.0 * cosw)
               if hit_s: hits |= 1 << s
               sum.c = sum.c + L.c * w                             float32 multiply, then float32 add
           indirect.c = sum.c / float32(K)
           bounce.c   = albedo.c * indirect.c
    miss, or max_trace_depth == 0:  hits = 0, indirect = bounce = +0, +0, +0

Nothing is traced or shaded here: the records of the primary rays, the spawned rays' records and colours and the albedo
are INPUTS (from the library's single-purpose queries, or from the oracle)."""
import numpy as np

import occlusion_reference as ocr

F32, F64, U64 = np.float32, np.float64, np.uint64
MAX_SAMPLES = 64


def spawned(records, dirs, idx, K, seed):
    """(hit (n,) bool, N (n, 3), rays (n, K, 6)): the K rays (from, res) of every sample; rows of misses are zeros"""
    hit, res, seg, _ = ocr.samples(records, dirs, idx, K, 1.0, seed)
    n = len(records)
    N = np.zeros((n, 3), dtype=F64)
    rays = np.zeros((n, K, 6), dtype=F64)
    if hit.any():
        N[hit] = ocr.faceforward(np.asarray(dirs, dtype=F64)[hit], records["normal"][hit])
        rays[hit] = np.concatenate([seg[hit][:, :, :3], res[hit]], axis=-1)
    return hit, N, rays


def weights(res, N):
    """w (n, K) float32 for directions res (n, K, 3) around N (n, 3)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (F64(2.0) * ocr.dot3(res, N[:, None, :])).astype(F32)


def planes(records, N, rays, sample_node, sample_rgb, albedo, K, depth0=False):
    """The four planes from the spawned rays of `spawned`, their closest nodes (n, K) and colours (n, K, 3) float32
    (rows of misses are not read) and the primary albedo (n, 3) float32"""
    n = len(records)
    hit = records["closest_node"] >= 0
    live = hit & (not depth0)
    w = weights(rays[:, :, 3:], N)
    L = np.asarray(sample_rgb, dtype=F32).reshape(n, K, 3)
    got = (np.asarray(sample_node).reshape(n, K) >= 0) & live[:, None]
    mask = np.zeros(n, dtype=U64)
    total = np.zeros((n, 3), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(K):
            mask[got[:, s]] |= U64(1 << s)
            term = (L[:, s, :] * w[:, s, None]).astype(F32)
            total[live] = (total[live] + term[live]).astype(F32)
        indirect = (total / F32(K)).astype(F32)
        indirect[~live] = 0
        bounce = (np.asarray(albedo, dtype=F32).reshape(n, 3) * indirect).astype(F32)
        bounce[~live] = 0
    return {"node": records["closest_node"].astype(np.int32), "hits": mask, "indirect": indirect, "bounce": bounce}


def mask_kinds(mask, hit, K):
    """(mixed, full, empty) among the hits"""
    return ocr.mask_kinds(mask, hit, K)

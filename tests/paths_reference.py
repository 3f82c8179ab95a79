"""A numpy restatement of the path planes' definition (include/c2rt.h, "path planes"), independent of the library: the
directions are tests/occlusion_reference.py's hemisphere samples under tests/camera_reference.py's rng_key(seed, idx, j)
(tap = depth, sample = path), and what is restated here is the walk and its fp32 arithmetic, in the types of the
definition:

    hit:   for p in 0 .. P-1:                               path-major ...
               from = from0;  N = N0
               for j in 0 .. Beff-1:                        ... bounce-minor
                   res  = hemisphere_sample(rng_key(seed, idx, j), p, N)
                   w    = float32(2.0 * ((res.x*N.x + res.y*N.y) + res.z*N.z))
                   T.c  = w if j == 0 else (T.c * a.c) * w  float32, two multiplies in this order
                   sum.c = sum.c + L.c * T.c                float32 multiply, then float32 add; for a miss too (L = +0)
                   if the segment missed: break
                   segments += 1;  a = albedo of the segment's hit;  N, from = those of the segment's hit
           indirect.c = sum.c / float32(P);  bounce.c = a0.c * indirect.c;  radiance.c = rgb.c + bounce.c
    miss, or Beff == 0:  segments = 0, indirect = bounce = +0, +0, +0, radiance = rgb

Nothing is traced or shaded here: the records, colours and albedos of the primary rays and of every segment are INPUTS
(from the library's single-purpose queries, from the oracle, or made by hand).  A walk goes depth by depth, because what
is asked at depth j + 1 depends on the answers at depth j:

    w = Walk(records, dirs, idx, P, Beff, seed)
    for j in range(Beff):
        rays = w.rays(j)                    # (m, 6): the segments of the paths still alive, in the order of w.alive()
        w.answers(j, nodes, rgb, albedo, normals, points)
    planes = w.planes(albedo0, rgb0)
"""
import numpy as np

import camera_reference as cr
import occlusion_reference as ocr

F32, F64, U32 = np.float32, np.float64, np.uint32
MAX_PATHS, MAX_BOUNCES = 64, 8


def directions(seed, idx, j, p, N):
    """hemisphere_sample(rng_key(seed, idx, j), p, N) for arrays idx (m,), p (m,), N (m, 3): (m, 3)"""
    key = cr.rng_key(int(seed), np.asarray(idx, dtype=np.uint64).reshape(-1), j)
    p = np.asarray(p, dtype=U32).reshape(-1)
    u, v = cr.rng_uniform(key, p, 0), cr.rng_uniform(key, p, 1)
    return ocr.flipped(ocr.unflipped(u, v), np.asarray(N, dtype=F64))[0]


def weight(res, N):
    """w (m,) float32 for directions res (m, 3) around N (m, 3)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (F64(2.0) * ocr.dot3(res, N)).astype(F32)


class Walk:
    def __init__(self, records, dirs, idx, P, beff, seed):
        assert 1 <= P <= MAX_PATHS and 0 <= beff <= MAX_BOUNCES
        self.n, self.P, self.beff, self.seed = len(records), int(P), int(beff), seed
        self.idx = np.asarray(idx, dtype=np.uint64).reshape(-1)
        self.node = records["closest_node"].astype(np.int32)
        self.hit = self.node >= 0
        self.live = self.hit & (self.beff != 0)
        n, P = self.n, self.P
        with np.errstate(invalid="ignore", over="ignore"):
            N0 = ocr.faceforward(np.asarray(dirs, dtype=F64), records["normal"])
            from0 = records["p"] + N0 * F64(1e-6)
        self.N = np.repeat(N0[:, None, :], P, axis=1)                 # (n, P, 3): every path starts at the primary hit
        self.origin = np.repeat(from0[:, None, :], P, axis=1)
        self.on = np.repeat(self.live[:, None], P, axis=1)            # (n, P): the path reaches the depth at hand
        self.T = np.zeros((n, P, 3), dtype=F32)
        self.a = np.zeros((n, P, 3), dtype=F32)
        self.term = np.zeros((n, P, max(self.beff, 1), 3), dtype=F32)  # L * T of every executed segment
        self.done = np.zeros((n, P, max(self.beff, 1)), dtype=bool)    # the segment was executed
        self.segments = np.zeros(n, dtype=np.uint32)
        self.hits_at = []                                              # hitting segments per depth
        self._res = None

    def alive(self):
        """(sample, path) of the paths that reach the depth at hand, sample-major"""
        return np.nonzero(self.on)

    def rays(self, j):
        s, p = self.alive()
        self._res = directions(self.seed, self.idx[s], j, p, self.N[s, p])
        return np.ascontiguousarray(np.concatenate([self.origin[s, p], self._res], axis=1))

    def answers(self, j, nodes, rgb, albedo, normals, points):
        """what c2rt_trace_rays (closest_node (m,), rgb (m, 3), normal, p) and the shading planes (albedo (m, 3)) say
        of the rays of rays(j); rows of misses are not read, but for their colour, which the caller gives as +0"""
        s, p = self.alive()
        res, N = self._res, self.N[s, p]
        w = weight(res, N)
        with np.errstate(invalid="ignore", over="ignore"):
            if j == 0:
                T = np.repeat(w[:, None], 3, axis=1)
            else:
                T = ((self.T[s, p] * self.a[s, p]).astype(F32) * w[:, None]).astype(F32)
            self.T[s, p] = T
            self.term[s, p, j] = (np.asarray(rgb, dtype=F32).reshape(-1, 3) * T).astype(F32)
        self.done[s, p, j] = True
        got = np.asarray(nodes).reshape(-1) >= 0
        np.add.at(self.segments, s[got], 1)
        self.hits_at.append(int(got.sum()))
        self.a[s, p] = np.asarray(albedo, dtype=F32).reshape(-1, 3)
        with np.errstate(invalid="ignore", over="ignore"):
            Nn = ocr.faceforward(res, np.asarray(normals, dtype=F64).reshape(-1, 3))
            self.N[s, p] = Nn
            self.origin[s, p] = np.asarray(points, dtype=F64).reshape(-1, 3) + Nn * F64(1e-6)
        self.on[s, p] = got

    def planes(self, albedo0, rgb0, order="path-major"):
        """the five planes; `order`: "path-major" is the definition's, "bounce-major" the other nest (for the test that
        the order matters)"""
        total = np.zeros((self.n, 3), dtype=F32)
        steps = [(p, j) for p in range(self.P) for j in range(self.beff)]
        if order != "path-major":
            steps = [(p, j) for j in range(self.beff) for p in range(self.P)]
        with np.errstate(invalid="ignore", over="ignore"):
            for p, j in steps:
                m = self.done[:, p, j]
                total[m] = (total[m] + self.term[m, p, j]).astype(F32)
            indirect = (total / F32(self.P)).astype(F32)
            indirect[~self.live] = 0
            bounce = (np.asarray(albedo0, dtype=F32).reshape(self.n, 3) * indirect).astype(F32)
            bounce[~self.live] = 0
            rgb0 = np.asarray(rgb0, dtype=F32).reshape(self.n, 3)
            radiance = np.where(self.live[:, None], (rgb0 + bounce).astype(F32), rgb0)
        return {"node": self.node, "segments": self.segments.copy(), "indirect": indirect, "bounce": bounce, "radiance": radiance}


def walk(records, dirs, idx, P, beff, seed, ask):
    """The whole walk with `ask(rays (m, 6)) -> (closest_node (m,), rgb (m, 3) float32, albedo (m, 3) float32, normal
    (m, 3), p (m, 3))` answering each depth's segments; returns the Walk (planes: .planes(albedo0, rgb0)) and, per depth,
    the rays asked"""
    w = Walk(records, dirs, idx, P, beff, seed)
    asked = []
    for j in range(w.beff):
        rays = w.rays(j)
        asked.append(rays)
        if not len(rays):
            w.hits_at.append(0)
            continue
        w.answers(j, *ask(rays))
    return w, asked

"""Shared by tests/test_ray_queries_abi.py (CPU) and tests/test_gpu_ray_queries.py (GPU): the ray oracle — the
reference's trace() loop restated over the oracle's exported Node.intersect — and the seeded ray sets."""
import ctypes as C

import numpy as np

import oracle_lib as orc
from chess2rt_amd import _abi
from chess2rt_amd.api import RAY_HIT_DTYPE


def _d3(a):
    return (C.c_double * 3)(*[float(v) for v in a])


def oracle_trace(desc, rays):
    """`trace` (rt/renderer.d:325-338) for each row of `rays` (n, 6): data.dist = 1e99, `foreach (node; scene.nodes)
    if (node.intersect(ray, data)) closestNode = node` — over ONE OrcHit, through orc_node_intersect.  Returns a
    RAY_HIT_DTYPE array; without a hit: -1, -1, 1e99 and zeros (what c2rt_ray_hit documents)."""
    L = orc.lib()
    d = desc.contents if hasattr(desc, "contents") else desc
    dp = C.pointer(d)
    out = np.zeros(len(rays), dtype=RAY_HIT_DTYPE)
    for i, r in enumerate(np.asarray(rays, dtype=np.float64)):
        o, v = _d3(r[:3]), _d3(r[3:])
        h = orc.OrcHit()
        h.dist = 1e99
        h.g = -1
        closest = -1
        for n in range(d.n_nodes):
            if L.orc_node_intersect(dp, n, o, v, C.byref(h)):
                closest = n
        rec = out[i]
        rec["closest_node"] = closest
        rec["dist"] = h.dist
        if closest >= 0:
            rec["leaf_geom"] = h.g
            rec["u"], rec["v"] = h.u, h.v
            rec["p"] = list(h.p)
            rec["normal"] = list(h.normal)
        else:
            rec["leaf_geom"] = -1
    return out


def oracle_visibility(desc, segments):
    L = orc.lib()
    d = desc.contents if hasattr(desc, "contents") else desc
    dp = C.pointer(d)
    return np.array([L.orc_test_visibility(dp, _d3(s[:3]), _d3(s[3:])) for s in np.asarray(segments, dtype=np.float64)], dtype=np.uint8)


def screen_rays(cam, width, height):
    """orc_screen_ray(cam, x, y) at every integer pixel, row-major: (W * H, 6)"""
    L = orc.lib()
    out = np.empty((height * width, 6), dtype=np.float64)
    o, v = (C.c_double * 3)(), (C.c_double * 3)()
    for y in range(height):
        for x in range(width):
            L.orc_screen_ray(C.byref(cam), float(x), float(y), o, v)
            out[y * width + x, :3] = list(o)
            out[y * width + x, 3:] = list(v)
    return out


def record_from_trace_result(t):
    """a c2rt_trace_result (probe / orc_render_pixel) as one RAY_HIT_DTYPE record, under c2rt_ray_hit's no-hit rule"""
    rec = np.zeros(1, dtype=RAY_HIT_DTYPE)[0]
    rec["closest_node"] = t.closest_node
    rec["dist"] = t.dist
    if t.closest_node >= 0:
        rec["leaf_geom"] = t.leaf_geom
        rec["u"], rec["v"] = t.u, t.v
        rec["p"] = list(t.p)
        rec["normal"] = list(t.normal)
    else:
        rec["leaf_geom"] = -1
    return rec


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_records_match_oracle(got, want, what=""):
    """The project's probe tolerances (tests/test_gpu_parity.py): node and leaf equal, dist and p bit for bit, normal
    within 1e-15, u, v within 1e-12 — with parity_util.maxdiff's rules for NaN and infinity."""
    from parity_util import maxdiff

    assert np.array_equal(got["closest_node"], want["closest_node"]), what
    assert np.array_equal(got["leaf_geom"], want["leaf_geom"]), what
    for f in ("dist", "p"):
        md, _, nne = maxdiff(got[f], want[f])
        assert md == 0.0 and nne == 0, (what, f, md, nne)
    with np.errstate(invalid="ignore"):
        def close(a, b, tol):
            a, b = a.astype(np.float64), b.astype(np.float64)
            same = (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & (a == b))
            return bool(np.all(same | (np.abs(a - b) <= tol)))
        assert close(got["normal"], want["normal"], 1e-15), (what, "normal")
        assert close(got["u"], want["u"], 1e-12) and close(got["v"], want["v"], 1e-12), (what, "u, v")


def scene_extent(desc):
    """(centre, half size) of the box around the scene's spheres and cubes (object space: good enough to aim at)"""
    d = desc.contents if hasattr(desc, "contents") else desc
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    prims = []
    for g in range(d.n_geoms):
        t = d.geom_type[g]
        if t in (_abi.GEOM_SPHERE, _abi.GEOM_CUBE):
            c = np.array([d.geom_param[4 * g + k] for k in range(3)])
            s = d.geom_param[4 * g + 3] * (1.0 if t == _abi.GEOM_SPHERE else 0.5)
            lo, hi = np.minimum(lo, c - s), np.maximum(hi, c + s)
            prims.append((t, c, d.geom_param[4 * g + 3]))
    if not prims:
        lo, hi = np.full(3, -50.0), np.full(3, 50.0)
    return (lo + hi) / 2, np.maximum((hi - lo) / 2, 10.0), prims


def eyeless_rays(desc, seed, n=2000):
    """Rays that share no eye (issue test 5): origins uniform in a box twice the scene's extent (inside solids, in
    cavities, below the ground); directions random unit vectors, half of them aimed at a primitive's centre so that
    small objects are hit at all; the six axis directions and directions with one zero component; lengths 0.5 and 3;
    origins exactly on a cube's face plane and on a sphere's surface."""
    rng = np.random.RandomState(seed)
    c, h, prims = scene_extent(desc)
    o = c + (rng.uniform(-2, 2, size=(n, 3)) * h)
    v = rng.normal(size=(n, 3))
    if prims:
        aim = rng.rand(n) < 0.5
        tgt = np.array([prims[k][1] for k in rng.randint(0, len(prims), size=n)]) + rng.normal(scale=2.0, size=(n, 3))
        v = np.where(aim[:, None], tgt - o, v)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    for k in range(36):
        v[5 + 11 * k] = axes[k % 6]
    for k in range(30):
        i = 9 + 13 * k
        v[i, k % 3] = 0.0
        v[i] /= np.linalg.norm(v[i])
    v[3::10] *= 0.5
    v[7::10] *= 3.0
    for k, (t, pc, size) in enumerate(prims[:20]):
        i = 1 + 17 * k
        if t == _abi.GEOM_CUBE:
            o[i] = pc + rng.uniform(-0.4, 0.4, size=3) * size
            o[i, k % 3] = pc[k % 3] + (0.5 if k % 2 else -0.5) * size      # exactly on a face plane (object space)
        else:
            u = rng.normal(size=3)
            o[i] = pc + u / np.linalg.norm(u) * size                      # on the sphere, up to rounding
    return np.ascontiguousarray(np.hstack([o, v]))


def csg_node_mask(desc):
    d = desc.contents if hasattr(desc, "contents") else desc
    return np.array([d.geom_type[d.node_geom[n]] >= _abi.GEOM_CSG_UNION for n in range(d.n_nodes)], dtype=bool)


def light_positions(desc):
    d = desc.contents if hasattr(desc, "contents") else desc
    return np.array([[d.light_pos[3 * l + k] for k in range(3)] for l in range(d.n_lights)], dtype=np.float64).reshape(-1, 3)


def visibility_segments(desc, records, seed, n_random=1000):
    """p + normal * 1e-6 of every hit towards every light, plus n_random point pairs in the scene's box"""
    lights = light_positions(desc)
    hit = records[records["closest_node"] >= 0]
    ok = np.isfinite(hit["p"]).all(axis=1) & np.isfinite(hit["normal"]).all(axis=1)
    frm = hit["p"][ok] + hit["normal"][ok] * 1e-6
    segs = [np.hstack([frm, np.broadcast_to(l, frm.shape)]) for l in lights]
    rng = np.random.RandomState(seed)
    c, h, _ = scene_extent(desc)
    a = c + rng.uniform(-1.2, 1.2, size=(n_random, 3)) * h
    b = c + rng.uniform(-1.2, 1.2, size=(n_random, 3)) * h
    a[:, 1] = np.abs(a[:, 1] - c[1]) + 0.5      # mostly above the ground: both answers occur
    b[:, 1] = np.abs(b[:, 1] - c[1]) + 0.5
    segs.append(np.hstack([a, b]))
    return np.ascontiguousarray(np.vstack(segs))

"""A typed restatement of the reference's GEOMETRY stage, independent of oracle/c2rt_oracle.c and of the device code: the
twin of tests/shade_reference.py.  Together they compute a frame with no oracle in it: rays -> records (`trace`) ->
visibility (`test_visibility`) -> colour (shade_reference.shade).

Written from the reference's D source (paths relative to its source/rt/): node.d:23-49 (Node.intersect),
transform.d:57-86 (point, undoPoint, direction, normal, undoDirection), imported_types.d:13-20,44-60 (mul, project,
unproject), geometry.d:30-59 (Plane), 92-130 (Sphere), 165-235 (Cube), 271-337 (CsgOp), 382-402 (CsgDiff),
intersectable.d:27-32 (opCmp on dist), renderer.d:325-338 (trace) and scene.d:62-78 (testVisibility).  gfm:math's vec3d
is not part of the reference's tree; its published algorithms are used: dot and squaredMagnitude are `sum = 0; sum +=
a_i * b_i`, magnitude is sqrt(squaredMagnitude), normalize is `v *= 1 / sqrt(squaredMagnitude)`.

Inputs are the scene descriptor's tables (include/c2rt.h) and rays / segments; nothing else.  Rules of evaluation:
  - every operation in np.float64, in source order, nothing fused (numpy never contracts);
  - mul(v, m) exactly as imported_types.d:15-19: a ROW vector times c[i][j];
  - the three matrices and the offset of a node are used AS GIVEN in node_transform; they are never recomputed;
  - a Plane's `limit` is geom_param[1]; the loader leaves it NaN (Plane() has no initialiser), and `fabs(p.x) > NaN` is
    false, which is what the comparisons below do with it;
  - Cube: the face pairs in the order Y, X (project 1, 0, 2), Z (project 0, 2, 1); `mult > data.dist` continues, so a
    later pair overrides an earlier one at EQUAL distance; u, v are taken in the projected frame;
  - findAllIntersections restarts from p + dir * 1e-6 and sums the lengths without those steps; it is capped at
    MAX_CSG_HITS hits per child as the ABI documents (the reference loops `while (true)`); `Trace.truncations` counts
    the lists that reached the cap (0 on tests/geom_scenes.py; one tree of tests/csg_edge_scenes.py is built to reach it);
  - the CsgOp walk sorts chain(leftData[], rightData[]) by dist with the reference's shell sort, restated literally
    from util/array.d:95-111 (`shell_sort`: gap n / 2, insertion by gap with the `ref i` index rewound by the inner
    `while`, `inc == 2 ? 1 : cast(int)(inc * 5.0 / 11)`, strict `>` on dist), which is NOT stable.  A comparison sort
    of DISTINCT keys has one result, so the rows whose stable order has no equal finite neighbours (and no NaN) are
    sorted by numpy's stable argsort, and only the others — the tied lists — go through the literal sort, row by
    row: the reference is defined on ties.  `Trace.ties` counts equal neighbouring distances in a sorted list, a
    statistic (tests/geom_scenes.py's tests require 0 on their scene; tests/csg_edge_scenes.py is built to have
    many).  Parities come from the list lengths; `current.g is left` compares the LEAF, so the entries of a nested
    CsgOp left child toggle inR, an entry of the right list whose leaf is `left` toggles inL, and in Op(a, a) every
    entry toggles inL; `data = current` copies the whole record;
  - per-ray flags of the walk (Trace.flags, and Trace.node_flags per node): tied_list (a sorted list with equal
    neighbours was walked), odd_list (a child list of odd length), long_list (a child list of more than two),
    capped_list, right_entry_toggles_left, left_entry_toggles_right (the last two for entries the walk visited);
  - sphere u, v are the one place with libm and the reference's 80-bit PI: they are evaluated with mpmath at 50 digits
    from the typed object-space p (the subtractions and the division by R in double, as written) and rounded ONCE; as
    nothing in the geometry stage reads u or v, this is done once, for the record that survives;
  - a miss is the record c2rt_ray_hit documents: node and leaf -1, dist 1e99, the rest 0.

Vectorised over rays; every statement acts on the rays its `if` lets through."""
import ctypes as C

import mpmath
import numpy as np

F64 = np.float64
GEOM_PLANE, GEOM_SPHERE, GEOM_CUBE, GEOM_CSG_UNION, GEOM_CSG_INTER, GEOM_CSG_DIFF = range(6)
MAX_CSG_HITS = 8            # C2RT_MAX_CSG_HITS, include/c2rt.h

# the named misreadings of test_geom_reference's mutation check (each changes ONE statement below)
GEOM_MUTATIONS = ("column_vector_product", "inverse_for_normal", "transform_for_undo", "normal_not_renormalised", "dist_not_rescaled",
                  "point_offset_before_matrix", "cube_uv_unprojected", "cube_equal_distance_keeps_first", "csg_identity_by_subtree",
                  "restart_length_includes_step", "diff_flip_probes_left", "plane_limit_ignored", "visibility_uses_1e99")
# those of test_csg_edge_reference's (tests/csg_edge_scenes.py: ties, shared leaves, Op(a, a), Plane operands): the chain
# is (right, left); `>=` in the sort's inner while; Plane.isInside true below the plane; inL, inR start false whatever the
# list lengths; in Op(a, a) the right list toggles inR
CSG_EDGE_MUTATIONS = ("chain_right_first", "sort_not_strict", "plane_is_inside_below", "parity_starts_outside", "op_aa_by_list")
MUTATIONS = GEOM_MUTATIONS + CSG_EDGE_MUTATIONS
# Variants that are REPORTED, not required to be seen: a stable sort in place of the shell sort (a trial over 50 tie trees
# changed no record: key patterns on which the two differ need a first hit equal to a second hit, and a second hit is a
# restart's 1e-6 short)
VARIANTS = ("stable_sort",)

RECORD = np.dtype([("closest_node", np.int32), ("leaf_geom", np.int32), ("dist", F64), ("u", F64), ("v", F64),
                   ("p", F64, 3), ("normal", F64, 3)])

# Hits.tag: which statement produced the surviving record
TAG_CUBE = {0: "cube -y", 1: "cube +y", 2: "cube -x", 3: "cube +x", 4: "cube -z", 5: "cube +z"}
TAG_SPHERE_NEAR, TAG_SPHERE_FAR, TAG_PLANE = 6, 7, 8


class Tables:
    """numpy copies of the descriptor fields the geometry stage reads (include/c2rt.h)"""

    def __init__(self, desc):
        d = desc.contents if hasattr(desc, "contents") else desc

        def arr(p, n, dt):
            return np.array([p[i] for i in range(n)], dtype=dt) if n else np.zeros(0, dtype=dt)
        ng, nn, nl = d.n_geoms, d.n_nodes, d.n_lights
        self.geom_type = arr(d.geom_type, ng, np.int64)
        self.geom_param = arr(d.geom_param, 4 * ng, F64).reshape(ng, 4)
        self.geom_child = arr(d.geom_child, 2 * ng, np.int64).reshape(ng, 2)
        self.node_geom = arr(d.node_geom, nn, np.int64)
        t = arr(d.node_transform, 30 * nn, F64).reshape(nn, 30)
        self.transform = t[:, 0:9].reshape(nn, 3, 3).copy()
        self.inverse = t[:, 9:18].reshape(nn, 3, 3).copy()
        self.transposed_inverse = t[:, 18:27].reshape(nn, 3, 3).copy()
        self.offset = t[:, 27:30].copy()
        self.light_pos = arr(d.light_pos, 3 * nl, F64).reshape(nl, 3)
        self.n_nodes, self.n_lights, self.n_geoms = nn, nl, ng


# ---- gfm:math vec3d, imported_types.d -------------------------------------------------------------------------------------


def dot(a, b):
    s = np.zeros(a.shape[:-1], dtype=F64)
    for i in range(3):
        s = s + a[..., i] * b[..., i]
    return s


def magnitude(v):
    return np.sqrt(dot(v, v))


def normalized(v):
    inv = F64(1) / np.sqrt(dot(v, v))
    return v * inv[..., None]


def mul(v, m, mut=None):
    """imported_types.d:13-20"""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    if mut == "column_vector_product":
        return np.stack([x * m[0][0] + y * m[0][1] + z * m[0][2],
                         x * m[1][0] + y * m[1][1] + z * m[1][2],
                         x * m[2][0] + y * m[2][1] + z * m[2][2]], axis=-1)
    return np.stack([x * m[0][0] + y * m[1][0] + z * m[2][0],
                     x * m[0][1] + y * m[1][1] + z * m[2][1],
                     x * m[0][2] + y * m[1][2] + z * m[2][2]], axis=-1)


# project(v, a, b, c): result[a] = v[0], result[b] = v[1], result[c] = v[2]; unproject: result[0] = v[a], ...
# (imported_types.d:44-60).  For (1, 0, 2) and (0, 2, 1) both are the same index list.
def project(v, a, b, c):
    out = np.empty_like(v)
    out[..., a], out[..., b], out[..., c] = v[..., 0], v[..., 1], v[..., 2]
    return out


def unproject(v, a, b, c):
    return np.stack([v[..., a], v[..., b], v[..., c]], axis=-1)


# ---- IntersectionData ---------------------------------------------------------------------------------------------------------


class Hits:
    """IntersectionData of n rays (intersectable.d:6-24; dNdx, dNdy are written by the reference and read by nothing on
    this path).  Besides the reference's fields: pobj, the object-space p of the sphere hit (for u, v); tag, flip, right:
    which statement made the record (cube face, sphere root; CsgDiff flipped the normal; the winning entry came from the
    right child's list of the outermost CsgOp) — for the tests' coverage conditions."""
    FIELDS = ("p", "normal", "dist", "u", "v", "g", "pobj", "tag", "flip", "right")

    def __init__(self, n, dist=1e99):
        self.p, self.normal, self.pobj = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        self.dist = np.full(n, dist, dtype=F64) if np.isscalar(dist) else np.array(dist, dtype=F64)
        self.u, self.v = np.zeros(n), np.zeros(n)
        self.g, self.tag = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        self.flip, self.right = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)

    def take(self, idx):
        out = Hits(0)
        for f in self.FIELDS:
            setattr(out, f, getattr(self, f)[idx].copy())
        return out

    def put(self, idx, other):
        for f in self.FIELDS:
            getattr(self, f)[idx] = getattr(other, f)


class Trace:
    """what one evaluation leaves behind: flags (name -> (n,) bool per input ray), node_flags ((name, node) -> the same
    for what happened under that node), truncations, ties and both per node"""

    def __init__(self, T, n, mut):
        self.T, self.mut, self.n = T, mut, n
        self.flags, self.node_flags = {}, {}
        self.truncations = 0
        self.ties = 0
        self.node = -1
        self.node_truncations = np.zeros(T.n_nodes, dtype=np.int64)
        self.node_ties = np.zeros(T.n_nodes, dtype=np.int64)

    def note(self, name, rows):
        self.flags.setdefault(name, np.zeros(self.n, dtype=bool))[rows] = True
        self.node_flags.setdefault((name, self.node), np.zeros(self.n, dtype=bool))[rows] = True

    def flag(self, name, node=None):
        z = np.zeros(self.n, dtype=bool)
        return self.flags.get(name, z) if node is None else self.node_flags.get((name, node), z)


# ---- geometry.d ---------------------------------------------------------------------------------------------------------------


def _plane(S, g, o, d, data, rows):
    """Plane.intersect, geometry.d:30-59"""
    y, limit = S.T.geom_param[g, 0], S.T.geom_param[g, 1]
    oy, dy = o[:, 1], d[:, 1]
    with np.errstate(all="ignore"):
        away = ((oy > y) & (dy > -1e-9)) | ((oy < y) & (dy < 1e-9))
        mult = (oy - y) / -dy
        ok = ~away & ~(mult > data.dist)
        p = o + d * mult[:, None]
        beyond = (np.abs(p[:, 0]) > limit) | (np.abs(p[:, 2]) > limit)
    S.note("plane_limit_rejects", rows[ok & beyond])
    if S.mut != "plane_limit_ignored":
        ok = ok & ~beyond
    data.p[ok] = p[ok]
    data.dist[ok] = mult[ok]
    data.normal[ok] = (0.0, 1.0, 0.0)
    data.u[ok], data.v[ok] = p[ok, 0], p[ok, 2]
    data.g[ok], data.tag[ok] = g, TAG_PLANE
    return ok


def _sphere(S, g, o, d, data, rows):
    """Sphere.intersect, geometry.d:92-125 (u, v: see sphere_uv)"""
    c, R = S.T.geom_param[g, :3], S.T.geom_param[g, 3]
    with np.errstate(all="ignore"):
        H = o - c
        A = dot(d, d)
        B = F64(2) * dot(H, d)
        Cq = dot(H, H) - R * R
        Dscr = B * B - F64(4) * A * Cq
        ok = ~(Dscr < 0)
        x1 = (-B + np.sqrt(Dscr)) / (F64(2) * A)
        x2 = (-B - np.sqrt(Dscr)) / (F64(2) * A)
        near = ~(x2 < 0)
        sol = np.where(near, x2, x1)
        ok = ok & ~(sol < 0) & ~(sol > data.dist)
        p = o + d * sol[:, None]
        nrm = normalized(p - c)
    data.dist[ok] = sol[ok]
    data.p[ok] = p[ok]
    data.normal[ok] = nrm[ok]
    data.pobj[ok] = p[ok]
    data.u[ok], data.v[ok] = 0.0, 0.0
    data.g[ok] = g
    data.tag[ok] = np.where(near[ok], TAG_SPHERE_NEAR, TAG_SPHERE_FAR)
    return ok


def _cube_side(S, side_len, o, d, c, data, pair):
    """Cube.intersectCubeSide, geometry.d:199-235"""
    with np.errstate(all="ignore"):
        live = ~(np.abs(d[:, 1]) < 1e-9)
        half = side_len * F64(0.5)
        found = np.zeros(len(o), dtype=bool)
        for side in (-1, 1):
            mult = (o[:, 1] - (c[1] + F64(side) * half)) / -d[:, 1]
            if S.mut == "cube_equal_distance_keeps_first":
                skip = (mult < 0) | (mult >= data.dist)
            else:
                skip = (mult < 0) | (mult > data.dist)
            p = o + d * mult[:, None]
            skip = skip | (p[:, 0] < c[0] - half) | (p[:, 0] > c[0] + half) | (p[:, 2] < c[2] - half) | (p[:, 2] > c[2] + half)
            ok = live & ~skip
            data.p[ok] = p[ok]
            data.dist[ok] = mult[ok]
            data.normal[ok] = (0.0, float(side), 0.0)
            data.u[ok] = p[ok, 0] - c[0]
            data.v[ok] = p[ok, 2] - c[2]
            data.tag[ok] = 2 * pair + (side > 0)
            found = found | ok
    return found


def _cube(S, g, o, d, data, rows):
    """Cube.intersect, geometry.d:172-197"""
    c, side_len = S.T.geom_param[g, :3], S.T.geom_param[g, 3]
    found = _cube_side(S, side_len, o, d, c, data, 0)
    for pair, (a, b, cc) in ((1, (1, 0, 2)), (2, (0, 2, 1))):
        f = _cube_side(S, side_len, project(o, a, b, cc), project(d, a, b, cc), project(c, a, b, cc), data, pair)
        data.normal[f] = unproject(data.normal[f], a, b, cc)
        data.p[f] = unproject(data.p[f], a, b, cc)
        if S.mut == "cube_uv_unprojected":
            data.u[f] = data.p[f, 0] - c[0]
            data.v[f] = data.p[f, 2] - c[2]
        found = found | f
    data.g[found] = g
    return found


def _bool_op(t, in_l, in_r):
    """geometry.d:361-364, 371-374, 399-402"""
    if t == GEOM_CSG_UNION:
        return in_l | in_r
    if t == GEOM_CSG_INTER:
        return in_l & in_r
    return in_l & ~in_r


def _find_all(S, geom, o, d, rows):
    """CsgOp.findAllIntersections, geometry.d:271-290 -> (entries: one full-length Hits per step, present (n, cap))"""
    n = len(o)
    origin = o.copy()
    length = np.zeros(n, dtype=F64)
    active = np.ones(n, dtype=bool)
    present = np.zeros((n, MAX_CSG_HITS), dtype=bool)
    entries = []
    for k in range(MAX_CSG_HITS):
        full = Hits(n)
        entries.append(full)
        idx = np.nonzero(active)[0]
        if not len(idx):
            continue
        temp = Hits(len(idx), 1e99)
        f = _geom(S, geom, origin[idx], d[idx], temp, rows[idx])
        active[idx[~f]] = False
        hit = idx[f]
        t = temp.take(np.nonzero(f)[0])
        t.dist = t.dist + length[hit]
        length[hit] = t.dist + F64(1e-6) if S.mut == "restart_length_includes_step" else t.dist
        origin[hit] = t.p + d[hit] * F64(1e-6)
        full.put(hit, t)
        present[hit, k] = True
    S.truncations += int(active.sum())          # these lists reached the cap
    S.node_truncations[S.node] += int(active.sum())
    S.note("capped_list", rows[active])
    return entries, present


def shell_sort(keys, strict=True):
    """util/array.d:95-111 on a list of keys -> the permutation it leaves (indices into `keys`).  `foreach (ref i, elem;
    arr)`: elem is a copy of arr[i] taken when the iteration starts, i is the loop's own index, so what the inner
    `while` takes off it is kept and the `foreach` goes on from there.  (`strict=False`, the misreading `>=`: with the
    rewound index two equal keys would change places for ever, so that variant inserts with an index of its own.)"""
    arr = list(range(len(keys)))
    inc = len(arr) // 2
    while inc:
        i = 0
        while i < len(arr):
            elem = arr[i]
            if strict:
                while i >= inc and keys[arr[i - inc]] > keys[elem]:
                    arr[i] = arr[i - inc]
                    i -= inc
                arr[i] = elem
                i += 1
            else:
                j = i
                while j >= inc and keys[arr[j - inc]] >= keys[elem]:
                    arr[j] = arr[j - inc]
                    j -= inc
                arr[j] = elem
                i += 1
        inc = 1 if inc == 2 else int(inc * 5.0 / 11)
    return arr


def _csg_base(S, g, o, d, data, rows):
    """CsgOp.intersect, geometry.d:292-332"""
    n = len(o)
    left, right = S.T.geom_child[g]
    le, lp = _find_all(S, left, o, d, rows)
    re, rp = _find_all(S, right, o, d, rows)
    entries, present = le + re, np.hstack([lp, rp])                 # chain(leftData[], rightData[])
    dist = np.full((n, 2 * MAX_CSG_HITS), np.inf)
    leaf = np.full((n, 2 * MAX_CSG_HITS), -1, dtype=np.int64)
    for k, e in enumerate(entries):
        dist[present[:, k], k] = e.dist[present[:, k]]
        leaf[:, k] = e.g
    chain = np.arange(2 * MAX_CSG_HITS)
    if S.mut == "chain_right_first":
        chain = np.concatenate([chain[MAX_CSG_HITS:], chain[:MAX_CSG_HITS]])
    order = chain[np.argsort(dist[:, chain], axis=1, kind="stable")]  # sort(allData[]) by opCmp: dist, where it has one result
    sd = np.take_along_axis(dist, order, axis=1)
    tied = np.isfinite(sd[:, 1:]) & (sd[:, 1:] == sd[:, :-1])
    S.ties += int(tied.sum())
    S.node_ties[S.node] += int(tied.sum())
    S.note("tied_list", rows[tied.any(axis=1)])
    if S.mut != "stable_sort":
        for r in np.nonzero(tied.any(axis=1) | (np.isnan(dist) & present).any(axis=1))[0]:      # util/array.d:95-111
            slots = chain[present[r, chain]]
            perm = shell_sort([dist[r, k] for k in slots], S.mut != "sort_not_strict")
            order[r, :len(slots)] = slots[perm]
            order[r, len(slots):] = chain[~present[r, chain]]
    nl, nr = lp.sum(axis=1), rp.sum(axis=1)
    S.note("odd_list", rows[(nl % 2 == 1) | (nr % 2 == 1)])
    S.note("long_list", rows[(nl > 2) | (nr > 2)])
    in_l = nl % 2 == 1
    in_r = nr % 2 == 1
    if S.mut == "parity_starts_outside":
        in_l, in_r = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    done = np.zeros(n, dtype=bool)
    chosen = np.full(n, -1, dtype=np.int64)
    ar = np.arange(n)
    for k in range(2 * MAX_CSG_HITS):
        slot = order[:, k]
        valid = present[ar, slot] & ~done
        if S.mut == "csg_identity_by_subtree" or (S.mut == "op_aa_by_list" and left == right):
            is_left = slot < MAX_CSG_HITS
        else:
            is_left = leaf[ar, slot] == left                         # `current.g is left`
        S.note("right_entry_toggles_left", rows[valid & is_left & (slot >= MAX_CSG_HITS)])
        S.note("left_entry_toggles_right", rows[valid & ~is_left & (slot < MAX_CSG_HITS)])
        in_l = np.where(valid & is_left, ~in_l, in_l)
        in_r = np.where(valid & ~is_left, ~in_r, in_r)
        fire = valid & _bool_op(S.T.geom_type[g], in_l, in_r)
        chosen[fire] = slot[fire]
        done = done | fire
    found = np.zeros(n, dtype=bool)
    for slot in np.unique(chosen[chosen >= 0]):
        r = np.nonzero(chosen == slot)[0]
        e = entries[slot]
        with np.errstate(invalid="ignore"):
            r = r[~(e.dist[r] > data.dist[r])]                       # `if (current.dist > data.dist) return false`
        data.put(r, e.take(r))                                       # `data = current`
        data.right[r] = slot >= MAX_CSG_HITS
        found[r] = True
    return found


def _csg_diff(S, g, o, d, data, rows):
    """CsgDiff.intersect, geometry.d:382-397"""
    found = _csg_base(S, g, o, d, data, rows)
    probe = S.T.geom_child[g][0 if S.mut == "diff_flip_probes_left" else 1]
    f = np.nonzero(found)[0]
    if len(f):
        step = d[f] * F64(1e-6)
        flip = is_inside(S.T, probe, data.p[f] - step, S.mut) != is_inside(S.T, probe, data.p[f] + step, S.mut)
        data.normal[f[flip]] = -data.normal[f[flip]]
        data.flip[f] = flip
    return found


def _geom(S, g, o, d, data, rows):
    t = S.T.geom_type[g]
    if t == GEOM_PLANE:
        return _plane(S, g, o, d, data, rows)
    if t == GEOM_SPHERE:
        return _sphere(S, g, o, d, data, rows)
    if t == GEOM_CUBE:
        return _cube(S, g, o, d, data, rows)
    if t == GEOM_CSG_DIFF:
        return _csg_diff(S, g, o, d, data, rows)
    return _csg_base(S, g, o, d, data, rows)


def is_inside(T, g, p, mut=None):
    """isInside, geometry.d:25-28 (Plane: false), 127-130 (Sphere: <), 165-170 (Cube: <=), 334-337 (CsgOp)"""
    t = T.geom_type[g]
    if t == GEOM_PLANE:
        if mut == "plane_is_inside_below":
            return p[:, 1] < T.geom_param[g, 0]
        return np.zeros(len(p), dtype=bool)
    c, s = T.geom_param[g, :3], T.geom_param[g, 3]
    with np.errstate(invalid="ignore"):
        if t == GEOM_SPHERE:
            q = c - p
            return dot(q, q) < s * s
        if t == GEOM_CUBE:
            h = s * F64(0.5)
            return (np.abs(p[:, 0] - c[0]) <= h) & (np.abs(p[:, 1] - c[1]) <= h) & (np.abs(p[:, 2] - c[2]) <= h)
    return _bool_op(t, is_inside(T, T.geom_child[g][0], p, mut), is_inside(T, T.geom_child[g][1], p, mut))


# ---- node.d, transform.d --------------------------------------------------------------------------------------------------


def point(T, node, p, mut=None):
    """Transform.point, transform.d:57-63"""
    if mut == "point_offset_before_matrix":
        return mul(p + T.offset[node], T.transform[node], mut)
    return mul(p, T.transform[node], mut) + T.offset[node]


def _node(S, node, o, d, data, rows):
    """Node.intersect, node.d:23-49"""
    T, mut = S.T, S.mut
    with np.errstate(all="ignore"):
        ro = mul(o - T.offset[node], T.inverse[node], mut)                                       # undoPoint
        rd = mul(d, T.transform[node] if mut == "transform_for_undo" else T.inverse[node], mut)  # undoDirection
        old = data.dist.copy()                                                                   # (1)
        length = magnitude(rd)
        if mut != "dist_not_rescaled":
            data.dist = data.dist * length                                                       # (2)
        rd = normalized(rd)                                                                      # (3)
        f = _geom(S, T.node_geom[node], ro, rd, data, rows)
        data.dist[~f] = old[~f]                                                                  # (4)
        nrm = mul(data.normal[f], T.inverse[node] if mut == "inverse_for_normal" else T.transposed_inverse[node], mut)
        data.normal[f] = nrm if mut == "normal_not_renormalised" else normalized(nrm)
        data.p[f] = point(T, node, data.p[f], mut)
        data.dist[f] = data.dist[f] / length[f]                                                  # (5)
    return f


# ---- sphere u, v: mpmath at 50 digits, rounded once ---------------------------------------------------------------------------

_MP = mpmath.mp.clone()
_MP.dps = 50


def _to_double(x):
    return mpmath.libmp.to_float(x._mpf_, rnd=mpmath.libmp.round_nearest)


def sphere_uv(c, R, p):
    """geometry.d:118-120 for one object-space p: angle = atan2(p.z - c.z, p.x - c.x); u = (PI + angle) / (2 PI);
    v = 1 - (PI / 2 + asin((p.y - c.y) / R)) / PI"""
    with np.errstate(all="ignore"):
        dz, dx, s = F64(p[2]) - c[2], F64(p[0]) - c[0], (F64(p[1]) - c[1]) / R
    pi = _MP.pi
    if not (np.isfinite(dz) and np.isfinite(dx)):
        u = float("nan")
    else:
        u = _to_double((pi + _MP.atan2(_MP.mpf(float(dz)), _MP.mpf(float(dx)))) / (2 * pi))
    if not (abs(s) <= 1):
        v = float("nan")
    else:
        v = _to_double(1 - (pi / 2 + _MP.asin(_MP.mpf(float(s)))) / pi)
    return u, v


# ---- renderer.d, scene.d ------------------------------------------------------------------------------------------------------


def trace(T, rays, mut=None):
    """Renderer.trace's closest-hit loop, renderer.d:325-338, for every row of `rays` (n, 6: origin, direction as given)
    -> (records of dtype RECORD, Trace).  Trace.hits holds the surviving Hits (tag, flip, right) per ray."""
    rays = np.asarray(rays, dtype=F64)
    n = len(rays)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    S = Trace(T, n, mut)
    rows = np.arange(n)
    data = Hits(n, 1e99)                                             # result.data.dist = 1e99
    closest = np.full(n, -1, dtype=np.int64)
    for node in range(T.n_nodes):                                    # foreach (node; scene.nodes)
        S.node = node
        f = _node(S, node, o, d, data, rows)
        closest[f] = node                                            # the last node that returns true
    hit = closest >= 0
    recs = np.zeros(n, dtype=RECORD)
    recs["closest_node"] = closest
    recs["leaf_geom"] = np.where(hit, data.g, -1)
    recs["dist"] = np.where(hit, data.dist, 1e99)
    for i in np.nonzero(hit & (T.geom_type[np.where(hit, data.g, 0)] == GEOM_SPHERE))[0]:
        g = data.g[i]
        data.u[i], data.v[i] = sphere_uv(T.geom_param[g, :3], T.geom_param[g, 3], data.pobj[i])
    recs["u"], recs["v"] = np.where(hit, data.u, 0.0), np.where(hit, data.v, 0.0)
    recs["p"] = np.where(hit[:, None], data.p, 0.0)
    recs["normal"] = np.where(hit[:, None], data.normal, 0.0)
    S.hits = data
    return recs, S


def test_visibility(T, segments, mut=None):
    """Scene.testVisibility, scene.d:62-78, for every row of `segments` (n, 6: from, to) -> (visible (n,) uint8,
    occluder (n,): the node that returned true, -1 where visible, Trace)"""
    seg = np.asarray(segments, dtype=F64)
    n = len(seg)
    frm, to = seg[:, :3].copy(), seg[:, 3:].copy()
    S = Trace(T, n, mut)
    with np.errstate(all="ignore"):
        d = normalized(to - frm)
        dist = np.full(n, 1e99) if mut == "visibility_uses_1e99" else magnitude(to - frm)
    data = Hits(n, dist)
    occluder = np.full(n, -1, dtype=np.int64)
    rows = np.arange(n)
    for node in range(T.n_nodes):
        idx = np.nonzero(occluder < 0)[0]                             # `return false` at the first node that hits
        if not len(idx):
            break
        sub = data.take(idx)
        S.node = node
        f = _node(S, node, frm[idx], d[idx], sub, rows[idx])
        data.put(idx, sub)
        occluder[idx[f]] = node
    return (occluder < 0).astype(np.uint8), occluder, S


test_visibility.__test__ = False      # not a pytest case

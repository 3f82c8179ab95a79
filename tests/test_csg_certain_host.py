"""csg_certain.h on the host (tests/csg_certain_check.cpp) against the literal lists of tests/geom_reference.py and against
the oracle's records and visibility (ray_query_util.oracle_trace, oracle_visibility).

For every ray the reference side is geom_reference's own findAllIntersections of both children and its CsgOp walk, with
the limit at 1e99: (hit, side, k) of the winning entry, its distance, and the flags tied_list / odd_list.  Required:
  - no certain answer differs from the reference's (hit, side, k), and a certain hit's distance lies within its bound;
  - a ray whose reference trace carries tied_list, or odd_list for any reason but the certain-inside state of a child,
    is unsure (an odd RIGHT list behind an empty left list of an Inter / Diff does not count: the staged decision
    answers "no hit" from the left child alone, as the literal code's kCsgShortA does, and never looks at it);
  - with every margin at zero the same operands give wrong certain answers (printed): the sets can fail;
  - the unsure share of the lecture5 screen set is at most 1e-3 (printed).
The oracle side (its ray trace is a Python loop over rays and nodes, so it runs on strided subsets: every constructed set
and the lecture5 screen and shadow rays, a few thousand rays each): where the oracle's closest node is the CsgOp's, a
certain answer is a hit on the same child within its bound; where it is another node, a certain hit lies behind that
node's; a certain "no hit" never has the CsgOp's node as the closest.  Visibility (what kBool answers): a segment that
ends behind a certain hit is occluded in the oracle, and a segment along a certain "no hit" ray on which the oracle's
trace finds nothing at all is visible.

Ray sets.  (1) lecture5.sdl at 1920x1080, five taps: EVERY sample inside the node's bound and the floor's shadow segment
of every pixel, in chunks.  (2) Union, Inter, Diff over (Cube, Sphere), (Sphere, Cube), (Sphere, Sphere), (Cube, Cube)
with the eye outside both, inside one and inside both children, 96x54 screens.  (3) 1.2e6 constructed rays aimed within
1e-9 .. 1e-3 of cube edges and corners, of the circles where the sphere meets the faces, of sphere tangents, from
origins within 1e-9 .. 1e-3 of a surface, and through two cubes that share a face plane.  (4) tests/csg_edge_scenes.py's
own trees and ray sets (scene "identity": shared face planes bit for bit, concentric and tangent children): its screen
rays, its eyeless rays and _tree_rays — axis-parallel rays, origins and directions IN a shared plane, origins ON a plane
— against every tree of two distinct Sphere / Cube children."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import geom_reference as gr  # noqa: E402
import ray_query_util as rq  # noqa: E402
import chess2rt_amd as c2  # noqa: E402
from chess2rt_amd import _abi  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
LIBPATH = os.path.join(ROOT, "tests", "libcsg_certain_check.so")
UNSURE, NOHIT, HIT = 0, 1, 2
AA = ((0.0, 0.0), (0.3, 0.3), (0.6, 0.0), (0.0, 0.6), (0.6, 0.6))
CUBE = (-100.0, 60.0, 200.0, 100.0)      # lecture5's own operands
SPHERE = (-100.0, 60.0, 200.0, 70.0)
_DP, _IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("tests/libcsg_certain_check.so is missing: run `make all` (build())")
    return C.CDLL(LIBPATH)


@pytest.fixture(scope="module")
def scene():
    s = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    s.setFrameSize(1920, 1080)
    return s


def csg_of(d):
    for n in range(d.n_nodes):
        g = d.node_geom[n]
        if d.geom_type[g] >= _abi.GEOM_CSG_UNION:
            return n, g, d.geom_child[2 * g], d.geom_child[2 * g + 1]
    raise AssertionError("no CsgOp node")


def set_tree(d, op, left, right):
    """lecture5's CsgOp rewritten in place: operator and both children as (is_sphere, params)"""
    n, g, l, r = csg_of(d)
    d.geom_type[g] = op
    for c, (sph, p) in ((l, left), (r, right)):
        d.geom_type[c] = _abi.GEOM_SPHERE if sph else _abi.GEOM_CUBE
        for i in range(4):
            d.geom_param[4 * c + i] = p[i]
    return n, g, l, r


def decide(lib, op, left, right, o, dirs, ms=1.0):
    n = len(o)
    o, dirs = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(dirs, dtype=np.float64)
    kind, side, k = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    dist, dl = np.zeros(n), np.zeros(n)
    lp, rp = (C.c_double * 4)(*left[1]), (C.c_double * 4)(*right[1])
    idx = op - _abi.GEOM_CSG_UNION
    lib.csg_certain_decide(idx, int(idx != 0), int(idx == 1), int(left[0]), lp, int(right[0]), rp, o.ctypes.data_as(_DP),
                           dirs.ctypes.data_as(_DP), C.c_int64(n), C.c_double(ms), kind.ctypes.data_as(_IP), side.ctypes.data_as(_IP),
                           k.ctypes.data_as(_IP), dist.ctypes.data_as(_DP), dl.ctypes.data_as(_DP))
    return kind, side, k, dist, dl


def reference(T, g, o, dirs, chunk=200000):
    """geom_reference's lists and walk -> hit, side, k, dist, tied, odd, and whether the odd lists are a child's ONE hit"""
    n = len(o)
    hit, side, k = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, np.int64)
    dist, tied, odd, odd_ok = np.full(n, 1e99), np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    left, right = T.geom_child[g]
    for a in range(0, n, chunk):
        oo, dd = np.ascontiguousarray(o[a:a + chunk]), np.ascontiguousarray(dirs[a:a + chunk])
        m = len(oo)
        rows = np.arange(m)
        S = gr.Trace(T, m, None)
        S.node = 0
        data = gr.Hits(m, 1e99)
        lists, find_all = [], gr._find_all

        def spy(*a):            # (the two lists _csg_base collects, left then right: the children are primitives)
            lists.append(find_all(*a))
            return lists[-1]

        gr._find_all = spy
        try:
            found = gr._csg_base(S, g, oo, dd, data, rows)
        finally:
            gr._find_all = find_all
        (le, lp), (re_, rp) = lists
        kk = np.zeros(m, np.int64)
        for s_, (ents, pres) in enumerate(((le, lp), (re_, rp))):
            for j, e in enumerate(ents):
                sel = found & (data.right == bool(s_)) & pres[:, j] & (e.dist == data.dist)
                kk[sel] = j
        nl, nr = lp.sum(axis=1), rp.sum(axis=1)
        sl = slice(a, a + m)
        hit[sl], side[sl], k[sl], dist[sl] = found, data.right.astype(np.int64), kk, data.dist
        tied[sl], odd[sl] = S.flag("tied_list"), S.flag("odd_list")
        # the certain-inside state: a child with exactly one hit (the origin inside it)
        l_one, r_one = nl == 1, nr == 1
        odd_ok[sl] = ((nl % 2 == 0) | l_one) & ((nr % 2 == 0) | r_one)
        # ... and a right list the staged decision never looks at: the left list is empty under an Inter or a Diff (the
        # exact shortcut kCsgShortA: no hit, whatever the right child's list is)
        if T.geom_type[g] != gr.GEOM_CSG_UNION:
            odd_ok[sl] |= (nl == 0)
    return hit, side, k, dist, tied, odd, odd_ok


def check(lib, T, g, op, left, right, o, dirs, what, oracle=None):
    """oracle: (desc, node, (left geometry, right geometry)) for the sets that also go through the oracle"""
    kind, side, k, dist, dl = decide(lib, op, left, right, o, dirs)
    if oracle is not None:
        oracle_check(oracle[0], oracle[1], oracle[2], np.asarray(o), np.asarray(dirs), kind, side, dist, dl, what)
    rh, rs, rk, rd, tied, odd, odd_ok = reference(T, g, o, dirs)
    sure = kind != UNSURE
    wrong = (sure & (rh != (kind == HIT))) | ((kind == HIT) & rh & ((rs != side) | (rk != k) | ~(np.abs(rd - dist) <= dl)))
    must_unsure = tied | (odd & ~odd_ok)
    print("%s: %d rays, %d unsure (%.2e), %d hits, %d tied, %d odd" % (what, len(o), int((~sure).sum()), (~sure).mean(), int(rh.sum()),
                                                                        int(tied.sum()), int(odd.sum())))
    assert not wrong.any(), (what, int(wrong.sum()), np.nonzero(wrong)[0][:5].tolist())
    assert not (must_unsure & sure).any(), (what, int((must_unsure & sure).sum()))
    # margins at zero: count the certain answers that are then wrong (reported by the caller)
    k0, s0, kk0, d0, _ = decide(lib, op, left, right, o, dirs, ms=0.0)
    wrong0 = ((k0 != UNSURE) & (rh != (k0 == HIT))) | ((k0 == HIT) & rh & ((rs != s0) | (rk != kk0)))
    return int((~sure).sum()), int(wrong0.sum()), sure


def oracle_check(desc, node, kids, o, v, kind, side, dist, dl, what, limit=4000):
    """a strided subset of the rays through the oracle's trace and visibility (world space = the node's object space)"""
    step = max(1, len(o) // limit)
    sel = np.arange(0, len(o), step)
    o, v, kind, side, dist, dl = o[sel], v[sel], kind[sel], side[sel], dist[sel], dl[sel]
    rec = rq.oracle_trace(desc, np.hstack([o, v]))
    own = rec["closest_node"] == node
    hit, nohit = kind == HIT, kind == NOHIT
    assert not (own & nohit).any(), (what, "the oracle hits the CsgOp where the answer is a certain miss", int((own & nohit).sum()))
    a = own & hit
    assert np.array_equal(rec["leaf_geom"][a], np.array(kids)[side[a]]), (what, "the oracle's leaf is the other child")
    assert (np.abs(rec["dist"][a] - dist[a]) <= dl[a]).all(), (what, "the oracle's distance is outside the bound")
    b = ~own & hit
    assert (rec["dist"][b] <= dist[b] + dl[b]).all(), (what, "the oracle sees nothing in front of a certain hit")
    # visibility: behind a certain hit -> occluded; along a certain miss on which the trace finds nothing -> visible
    length = np.where(hit, dist + dl + 1.0, 1000.0)
    vis = rq.oracle_visibility(desc, np.hstack([o, o + v * length[:, None]]))
    assert not vis[hit].any(), (what, "visible through a certain hit", int(vis[hit].sum()))
    free = nohit & (rec["closest_node"] < 0)
    assert vis[free].all(), (what, "occluded where nothing is hit")
    print("%s: oracle: %d rays, %d closest on the CsgOp, %d certain hits behind another node, %d free" % (what, len(o), int(a.sum()), int(b.sum()),
                                                                                                       int(free.sum())))
    return int(a.sum())


def cam_vectors(cam):
    g = lambda f: np.array([getattr(cam, f)[i] for i in range(3)])
    return g("pos"), g("up_left"), g("up_right"), g("down_left")


def screen_dirs(cam, W, H, taps):
    pos, ul, ur, dl = cam_vectors(cam)
    out = []
    for (ax, ay) in AA[:taps]:
        xs, ys = np.meshgrid(np.arange(W) + ax, np.arange(H) + ay)
        v = ul + (ur - ul) * (xs / W)[..., None] + (dl - ul) * (ys / H)[..., None] - pos
        v = v.reshape(-1, 3)
        out.append(v / np.linalg.norm(v, axis=1, keepdims=True))
    return pos, np.vstack(out)


def floor_shadow(pos, dirs, floor_y, light):
    """the floor's shadow segments: from p + N 1e-6 towards the light, for the rays that reach the floor"""
    down = dirs[:, 1] < -1e-9
    t = (pos[1] - floor_y) / -dirs[down, 1]
    p = pos + dirs[down] * t[:, None]
    frm = p + np.array([0.0, 1e-6, 0.0])
    v = light - frm
    return frm, v / np.linalg.norm(v, axis=1, keepdims=True)


def near(mask, reach=50):
    idx = np.nonzero(mask)[0]
    out = np.zeros(len(mask), bool)
    for s in range(-reach, reach + 1):
        j = idx + s
        out[j[(j >= 0) & (j < len(mask))]] = True
    return out


def test_lecture5_screen_and_shadow_rays(lib, scene):
    d = scene.desc.contents
    cam = scene.beginFrame()
    n, g, l, r = csg_of(d)
    T = gr.Tables(scene.desc)
    left, right = (False, CUBE), (True, SPHERE)
    assert tuple(d.geom_param[4 * l + i] for i in range(4)) == CUBE and tuple(d.geom_param[4 * r + i] for i in range(4)) == SPHERE
    pos, dirs = screen_dirs(cam, 1920, 1080, 5)
    c, rad = np.array(CUBE[:3]), CUBE[3] * 0.5 * np.sqrt(3.0) * 1.001     # the node's bound: the left child's sphere
    H = pos - c
    b = dirs @ H
    inside = b * b - (H @ H - rad * rad) > 0
    o_all = np.broadcast_to(pos, dirs.shape)
    light = np.array([d.light_pos[i] for i in range(3)])
    sf, sd = floor_shadow(pos, dirs[:1920 * 1080], d.geom_param[0], light)
    total = unsure = wrong0 = 0
    for what, o, v in (("primary", o_all[inside], dirs[inside]), ("floor shadow", sf, sd)):
        u, w0, _ = check(lib, T, g, _abi.GEOM_CSG_DIFF, left, right, o, v, "lecture5 1920x1080 x5 " + what, oracle=(scene.desc, n, (l, r)))
        total += len(o)
        unsure += u
        wrong0 += w0
    share = unsure / total
    print("lecture5 screen set: %d rays, unsure share %.3e; wrong certain answers with every margin at zero: %d" % (total, share, wrong0))
    assert share <= 1e-3


PAIRS = {"cube_sphere": ((False, CUBE), (True, SPHERE)), "sphere_cube": ((True, SPHERE), (False, CUBE)),
         "sphere_sphere": ((True, (-100.0, 60.0, 200.0, 60.0)), (True, (-60.0, 80.0, 170.0, 50.0))),
         "cube_cube": ((False, CUBE), (False, (-60.0, 90.0, 160.0, 90.0)))}
EYES = {"outside": (0.0, 165.0, 0.0), "inside_one": (-140.0, 20.0, 240.0), "inside_both": (-90.0, 70.0, 190.0)}


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("op", [_abi.GEOM_CSG_UNION, _abi.GEOM_CSG_INTER, _abi.GEOM_CSG_DIFF])
def test_scene_variants(lib, op, pair):
    s = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    s.setFrameSize(96, 54)
    d = s.desc.contents
    left, right = PAIRS[pair]
    n, g, l, r = set_tree(d, op, left, right)
    T = gr.Tables(s.desc)
    cam = s.beginFrame()
    _, dirs = screen_dirs(cam, 96, 54, 5)
    light = np.array([d.light_pos[i] for i in range(3)])
    certain = 0
    for eye_name, eye in sorted(EYES.items()):
        eye = np.array(eye)
        aim = np.array(CUBE[:3]) - eye      # look at the solid from wherever the eye is
        aim /= np.linalg.norm(aim)
        fwd = np.array([cam.front_dir[i] for i in range(3)]) if hasattr(cam, "front_dir") else np.array([0.0, 0.0, 1.0])
        # rotate the screen's directions so that the camera's axis points at the solid (any rotation will do: the rays only
        # have to sweep both children from this eye)
        v = np.cross(fwd, aim)
        cth = float(fwd @ aim)
        K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        R = np.eye(3) + K + K @ K / (1.0 + cth)
        dd = dirs @ R.T
        dd /= np.linalg.norm(dd, axis=1, keepdims=True)
        o = np.broadcast_to(eye, dd.shape)
        sf, sd = floor_shadow(eye if eye[1] > 1 else np.array([eye[0], 165.0, eye[2]]), dd[:96 * 54], d.geom_param[0], light)
        for what, oo, vv in ((eye_name, o, dd), (eye_name + " floor shadow", sf, sd)):
            if len(oo):
                u, _, sure = check(lib, T, g, op, left, right, oo, vv, "%s op %d %s" % (pair, op, what))
                certain += int(sure.sum())
    assert certain > 1000, "vacuous: nothing was certain"


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def constructed_rays(rng, n_each):
    """rays aimed within eps of the places where the stepped lists change class, eps log-uniform in [1e-9, 1e-3]"""
    lo, hi = np.array(CUBE[:3]) - CUBE[3] / 2, np.array(CUBE[:3]) + CUBE[3] / 2
    c, Rs = np.array(SPHERE[:3]), SPHERE[3]
    eps = lambda m: 10.0 ** rng.uniform(-9, -3, size=m) * rng.choice([-1.0, 1.0], size=m)
    origin = lambda m: np.array(CUBE[:3]) + _unit(rng.normal(size=(m, 3))) * rng.uniform(150, 400, size=(m, 1))
    sets = []
    m = n_each
    # cube edges: a point of an edge, displaced by eps along both face normals
    ax = rng.randint(0, 3, size=m)
    t = np.where(rng.rand(m, 3) < 0.5, lo, hi)
    along = rng.uniform(0, 1, size=m)
    t[np.arange(m), ax] = lo[ax] + along * (hi - lo)[ax]
    t += np.stack([eps(m), eps(m), eps(m)], axis=1) * (np.arange(3)[None, :] != ax[:, None])
    o = origin(m)
    sets.append((o, _unit(t - o)))
    # corners
    t = np.where(rng.rand(m, 3) < 0.5, lo, hi) + np.stack([eps(m), eps(m), eps(m)], axis=1)
    o = origin(m)
    sets.append((o, _unit(t - o)))
    # the circles where the sphere meets the cube's faces
    ax = rng.randint(0, 3, size=m)
    side = np.where(rng.rand(m) < 0.5, lo[ax], hi[ax])
    h = side - c[ax]
    rho = np.sqrt(np.maximum(Rs * Rs - h * h, 0.0))
    ang = rng.uniform(0, 2 * np.pi, size=m)
    t = np.tile(c, (m, 1))
    a1, a2 = (ax + 1) % 3, (ax + 2) % 3
    t[np.arange(m), ax] = side + eps(m)
    t[np.arange(m), a1] += (rho + eps(m)) * np.cos(ang)
    t[np.arange(m), a2] += (rho + eps(m)) * np.sin(ang)
    o = origin(m)
    sets.append((o, _unit(t - o)))
    # sphere tangents: aim at a point at distance R + eps from the centre, perpendicular to the line of sight
    o = origin(m)
    w = _unit(c - o)
    u = _unit(np.cross(w, rng.normal(size=(m, 3))))
    dist = np.linalg.norm(c - o, axis=1)
    Rt = Rs + eps(m)
    t = o + w * (dist - Rt * Rt / dist)[:, None] + u * (Rt * np.sqrt(1 - (Rt / dist) ** 2))[:, None]
    sets.append((o, _unit(t - o)))
    # origins within eps of a surface: on a cube face, on the sphere
    ax = rng.randint(0, 3, size=m)
    o = lo + rng.uniform(0, 1, size=(m, 3)) * (hi - lo)
    o[np.arange(m), ax] = np.where(rng.rand(m) < 0.5, lo[ax], hi[ax]) + eps(m)
    sets.append((o, _unit(rng.normal(size=(m, 3)))))
    o = c + _unit(rng.normal(size=(m, 3))) * (Rs + eps(m))[:, None]
    sets.append((o, _unit(rng.normal(size=(m, 3)))))
    return sets


def test_constructed_rays(lib, scene):
    d = scene.desc.contents
    T = gr.Tables(scene.desc)
    n, g, l, r = csg_of(d)
    rng = np.random.RandomState(20261020)
    total = wrong0 = 0
    names = ("cube edges", "cube corners", "sphere / face circles", "sphere tangents", "origins on a cube face", "origins on the sphere")
    for name, (o, v) in zip(names, constructed_rays(rng, 170000)):
        u, w0, _ = check(lib, T, g, _abi.GEOM_CSG_DIFF, (False, CUBE), (True, SPHERE), o, v, "constructed: " + name, oracle=(scene.desc, n, (l, r)))
        total += len(o)
        wrong0 += w0
    # two cubes that share a face plane (tests/csg_edge_scenes.py's shared-plane trees): every ray through both ties there
    s = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    dd = s.desc.contents
    A, B = (False, (-100.0, 60.0, 200.0, 100.0)), (False, (0.0, 60.0, 200.0, 100.0))       # A's +x face is B's -x face
    for op in (_abi.GEOM_CSG_UNION, _abi.GEOM_CSG_INTER, _abi.GEOM_CSG_DIFF):
        n, g, l, r = set_tree(dd, op, A, B)
        T2 = gr.Tables(s.desc)
        m = 60000
        o = np.array([-50.0, 60.0, 200.0]) + _unit(rng.normal(size=(m, 3))) * rng.uniform(200, 400, size=(m, 1))
        t = np.array([-50.0, 60.0, 200.0]) + rng.uniform(-1, 1, size=(m, 3)) * np.array([0.0, 50.0, 50.0])
        t[:, 0] += 10.0 ** rng.uniform(-9, -3, size=m) * rng.choice([-1.0, 1.0], size=m)
        u, w0, _ = check(lib, T2, g, op, A, B, o, _unit(t - o), "shared face plane, op %d" % op, oracle=(s.desc, n, (l, r)))
        total += m
        wrong0 += w0
    print("constructed rays: %d; wrong certain answers with every margin at zero: %d" % (total, wrong0))
    assert total >= 1000000
    assert wrong0 > 0, "the sets cannot fail: with no margin nothing came out wrong"


def test_csg_edge_scenes_ray_sets(lib):
    """tests/csg_edge_scenes.py, scene "identity": every depth-1 tree over two distinct Sphere / Cube children, with the
    scene's own screen and eyeless rays and _tree_rays' kinds (axis-parallel, in a shared plane, on a plane), normalised as
    Node.intersect normalises them; its Plane, Op(a, a) and nested trees are not served (tests/test_csg_certain_plan.py)"""
    import csg_edge_scenes as E

    case = E.load("identity")
    T = gr.Tables(case.desc)
    d = case.desc
    world = np.vstack([E.ray_set("identity", "screen"), E.ray_set("identity", "eyeless")])
    rng = np.random.RandomState(7)
    ops = {"U": _abi.GEOM_CSG_UNION, "I": _abi.GEOM_CSG_INTER, "D": _abi.GEOM_CSG_DIFF}
    served = tied = sure_total = 0
    for i, (name, tree, centre, s_, _, _) in enumerate(E.TREES["identity"]):
        node = i + 1
        g = d.node_geom[node]
        l, r = d.geom_child[2 * g], d.geom_child[2 * g + 1]
        kinds = [d.geom_type[c] for c in (l, r)]
        if l == r or any(k not in (_abi.GEOM_SPHERE, _abi.GEOM_CUBE) for k in kinds):
            continue
        assert d.geom_type[g] == ops[tree[0]]
        left, right = [(d.geom_type[c] == _abi.GEOM_SPHERE, tuple(d.geom_param[4 * c + j] for j in range(4))) for c in (l, r)]
        gen, rest = E._tree_rays(rng, tree, centre, s_, 4000)
        rays = np.vstack([world, gen, rest])
        rays = rays[np.isfinite(rays).all(axis=1) & (np.linalg.norm(rays[:, 3:], axis=1) > 0)]
        o, v = np.ascontiguousarray(rays[:, :3]), _unit(rays[:, 3:])
        u, w0, sure = check(lib, T, g, d.geom_type[g], left, right, o, v, "csg_edge identity / " + name,
                            oracle=(case.desc, node, (l, r)))
        served += 1
        sure_total += int(sure.sum())
    assert served >= 10 and sure_total > 10000

"""Build-authored scenes and seeded ray sets for tests/test_csg_edge_reference.py (CPU) and tests/test_gpu_csg_edge.py:
CsgOp trees whose children share face planes bit for bit, share leaves, are the same leaf twice (Op(a, a)), have a Plane
as an operand, go to depth 4 and reach the build-defined cap of 8 hits per child — what the CsgOp walk of
rt/geometry.d:292-337 does with ties, odd hit counts and leaf identity, which tests/geom_scenes.py stays clear of.

Built the way geom_scenes.py is: the text goes through the host loader, the descriptor is COPIED, and (scene "placed")
three rows of node_transform are replaced by true rotations from c2rt_host_transform_rotate.  Reads
tests/golden/scenes/floor.bmp only.  61x47, object scale ~10, two lights.

Every tree has primitives of its own, with INTEGER centres and EVEN sides, so that `c +- side * 0.5` is exact and the
shared planes are the same doubles in both children.  Around a tree's centre (X, Y, Z) with side s, h = s / 2:
   a  Cube (X, Y, Z; s)                       b  Cube (X - s, Y, Z; s): shares a's face plane x = X - h, and its y and z planes
   e  Cube (X, Y + 2 (s / 5), Z; s): shares a's x and z planes             c  Cube (X, Y, Z; s - 4): concentric
   t  Sphere (X, Y, Z; R h): tangent to a's faces from inside              P  Plane y = Y (Q: y = Y - h - 1, below a)
   s  Sphere (X, Y - h + 2, Z - h; R 3): across a's front face             A0..A6, K  the cap tree's spheres (CAP_SPHERES)
   k  Sphere (X, Y + 5, Z; R 2)
A tree is ("U" | "I" | "D", left, right) over these letters; a letter used twice in one tree is ONE geometry.

Scene "identity": every node is the identity with zero offset (the identity-matrix instances; no tree here is a
CsgDiff(., Sphere), so the void-tile pre-pass registers none of them), the trees are placed by their centres.  Scene
"placed": trees around the origin of their object space under scale, the loader's `rotate` (a second scale,
rt/node.d:89-90), translate, and true rotations; its cap tree (CAP_TREE) lies along one pixel's ray under the identity."""
import ctypes as C
import functools
import os
import shutil
import tempfile

import numpy as np

import chess2rt_amd as c2
import geom_reference as gr
from chess2rt_amd import _abi
from golden_configs import SCENES
from ray_query_util import screen_rays

W, H = 61, 47
SCENE_NAMES = ("identity", "placed")
RAY_SETS = ("screen", "eyeless")
EYELESS_SEED, N_EYELESS = 41, 2048
GROUND = 0

# (name, tree, (X, Y, Z), s[, the node's text, true rotation: (angles, scale or None, offset)])
AE, EA, AB = ("a", "e"), ("e", "a"), ("a", "b")
IDENTITY_TREES = [
    ("diff_ae", ("D",) + AE, (-13, 13, -14), 20), ("diff_ab", ("D",) + AB, (23, 13, -14), 20),
    ("union_ae", ("U",) + AE, (-36, 8, 10), 10), ("inter_ae", ("I",) + AE, (-20, 8, 10), 10),
    ("union_ea", ("U",) + EA, (-4, 8, 10), 10), ("inter_ea", ("I",) + EA, (12, 8, 10), 10), ("diff_ea", ("D",) + EA, (28, 8, 10), 10),
    ("diff_a_plane", ("D", "a", "P"), (46, 10, 10), 14),
    ("inter_ab", ("I",) + AB, (-34, 8, 29), 10), ("diff_ba", ("D", "b", "a"), (-10, 8, 29), 10),
    ("union_aa", ("U", "a", "a"), (6, 8, 29), 10), ("inter_aa", ("I", "a", "a"), (22, 8, 29), 10), ("diff_aa", ("D", "a", "a"), (38, 8, 29), 10),
    ("diff_a_conc", ("D", "a", "c"), (-40, 10, 50), 14), ("inter_a_tangent", ("I", "a", "t"), (-18, 10, 50), 14),
    ("inter_plane_a", ("I", "P", "a"), (6, 12, 50), 18), ("diff_plane_a", ("D", "Q", "a"), (32, 10, 50), 14),
]
UAB, UAE = ("U", "a", "b"), ("U", "a", "e")
# The cap tree.  Disjoint operands cannot fill a hit list: a CsgUnion entered from inside a child reports the next ENTRY,
# not the exit, and the entries of a CsgOp left child toggle inR.  OVERLAPPING spheres on one axis can: the intervals
# below are where each sphere cuts the axis (in axis units of CAP_UNIT world units, from CAP_T0 along the screen ray of
# one pixel of the "placed" camera, so that this pixel's ray — and rays along it in the eyeless set — run down the axis).
CAP_SPHERES = {"A0": (56, 94), "A6": (44, 95), "A1": (6, 34), "A4": (37, 118), "A5": (57, 62), "K": (130, 134)}
CAP_TREE = ("U", ("U", ("U", ("U", "A0", "A6"), "A1"), ("U", ("U", "A4", "A5"), "A1")), "K")
CAP_UNIT, CAP_TARGET = 0.4, (0.0, 18.0, 20.0)
O = (0, 0, 0)
PLACED_TREES = [
    ("union_a_uab", ("U", "a", UAB), O, 10, "scale 1.25 0.75 1.5; translate -27 10 -12", None),
    ("inter_uab_a", ("I", UAB, "a"), O, 10, "rotate 0.75 1.5 1.25; translate -5 12 -12", None),
    ("diff_uab_uae", ("D", UAB, UAE), O, 10, "", ((25.0, 15.0, -30.0), None, (12.0, 14.0, -8.0))),
    ("depth4", ("D", ("I", ("D", UAB, "e"), UAE), "s"), O, 10, "", ((-20.0, 25.0, 10.0), (1.75, 1.75, 1.75), (31.0, 16.0, -12.0))),
    ("cap", CAP_TREE, CAP_TARGET, 10, "", None),
    ("diff_ae", ("D",) + AE, O, 10, "", ((35.0, -20.0, 15.0), None, (-36.0, 14.0, 22.0))),
    ("inter_ae", ("I",) + AE, O, 10, "scale 1.5 1.25 0.75; rotate 1 0.5 1; translate 36 12 24", None),
]
TREES = {"identity": [t + ("", None) for t in IDENTITY_TREES], "placed": PLACED_TREES}
# the two depth-1 tie trees whose regular / irregular 64-ray groups open the eyeless set
GROUP_TREES = {"identity": ("diff_ae", "union_ae"), "placed": ("diff_ae", "inter_ae")}
GROUPS = 4                   # [0, 64): all regular on tree 0; [64, 128): one irregular among 63; the same for tree 1
CAMERA = {"identity": "pos 2 78 -44; yaw 0; pitch -56; roll 0; fov 62", "placed": "pos 2 64 -52; yaw 0; pitch -46; roll 0; fov 62"}
LIGHTS = {"identity": ((-50.0, 70.0, -40.0), (70.0, 60.0, 20.0)), "placed": ((-40.0, 60.0, -40.0), (60.0, 50.0, 0.0))}

_TMP = tempfile.mkdtemp(prefix="c2rt_csg_edge_")
shutil.copy(os.path.join(SCENES, "floor.bmp"), os.path.join(_TMP, "floor.bmp"))


def node_index(scene, name):
    return 1 + [t[0] for t in TREES[scene]].index(name)


@functools.lru_cache(maxsize=None)
def cap_axis():
    """(origin, unit direction, t0) of the cap tree's axis: the screen ray of the pixel of the "placed" camera that passes
    nearest CAP_TARGET, from a scene that holds the camera and the ground only; axis unit x lies at t0 + x * CAP_UNIT"""
    path = os.path.join(_TMP, "csg_edge_camera.sdl")
    with open(path, "w") as f:
        f.write('Scene { GlobalSettings { frameWidth %d; frameHeight %d; AAEnabled false }\n Camera { %s }\n'
                ' Lights { PointLight "l" { pos 0 50 0; color 1 1 1; power 100 } }\n Geometries { Plane "g" { y 0 } }\n'
                ' Shaders { Lambert "s" { color 1 1 1 } }\n Nodes { Node "n" { geometry "g"; shader "s" } } }\n' % (W, H, CAMERA["placed"]))
    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    scene.setAA(False)
    scene.setDof(False)
    rays = screen_rays(scene.beginFrame(), W, H)
    o, d = rays[:, :3], rays[:, 3:] / np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    t = ((np.array(CAP_TARGET) - o) * d).sum(axis=1)
    k = int(np.argmin(np.linalg.norm(o + d * t[:, None] - np.array(CAP_TARGET), axis=1)))
    lo, hi = min(v[0] for v in CAP_SPHERES.values()), max(v[1] for v in CAP_SPHERES.values())
    return o[k].copy(), d[k].copy(), float(t[k]) - 0.5 * (lo + hi) * CAP_UNIT, k


def leaf_text(letter, name, X, Y, Z, s):
    h = s // 2
    if letter in CAP_SPHERES:
        o, d, t0, _ = cap_axis()
        lo, hi = CAP_SPHERES[letter]
        c = o + d * (t0 + 0.5 * (lo + hi) * CAP_UNIT)
        return 'Sphere "%s" { center %r %r %r; R %r }' % (name, float(c[0]), float(c[1]), float(c[2]), 0.5 * (hi - lo) * CAP_UNIT)
    if letter == "a":
        return 'Cube "%s" { center %d %d %d; side %d }' % (name, X, Y, Z, s)
    if letter == "b":
        return 'Cube "%s" { center %d %d %d; side %d }' % (name, X - s, Y, Z, s)
    if letter == "e":
        return 'Cube "%s" { center %d %d %d; side %d }' % (name, X, Y + 2 * (s // 5), Z, s)
    if letter == "c":
        return 'Cube "%s" { center %d %d %d; side %d }' % (name, X, Y, Z, s - 4)
    if letter == "t":
        return 'Sphere "%s" { center %d %d %d; R %d }' % (name, X, Y, Z, h)
    if letter == "s":
        return 'Sphere "%s" { center %d %d %d; R 3 }' % (name, X, Y - h + 2, Z - h)
    if letter == "k":
        return 'Sphere "%s" { center %d %d %d; R 2 }' % (name, X, Y + 5, Z)
    if letter == "P":
        return 'Plane "%s" { y %d }' % (name, Y)
    if letter == "Q":
        return 'Plane "%s" { y %d }' % (name, Y - h - 1)
    raise ValueError(letter)


def tree_text(name, tree, centre, s):
    """the geometries of one tree, leaves first -> (lines, {letter or root: geometry name})"""
    lines, names = [], {}

    def walk(t):
        if isinstance(t, str):
            if t not in names:
                names[t] = "%s_%s" % (name, t)
                lines.append(leaf_text(t, names[t], centre[0], centre[1], centre[2], s))
            return names[t]
        l, r = walk(t[1]), walk(t[2])
        op = "%s_op%d" % (name, len(lines))
        lines.append('%s "%s" { left "%s"; right "%s" }' % ({"U": "CsgUnion", "I": "CsgInter", "D": "CsgDiff"}[t[0]], op, l, r))
        return op
    names["root"] = walk(tree)
    return lines, names


def scene_text(scene):
    geoms, nodes = ['Plane "ground" { y 0 }'], ['Node "n0" { geometry "ground"; shader "sh_ground" }']
    shaders = ("sh_a", "sh_b", "sh_c", "sh_d", "sh_e")
    for i, (name, tree, centre, s, place, _) in enumerate(TREES[scene]):
        lines, names = tree_text(name, tree, centre, s)
        geoms += lines
        nodes.append('Node "n%d" { geometry "%s"; shader "%s"%s }' % (i + 1, names["root"], shaders[i % 5], "; " + place if place else ""))
    lights = ['PointLight "l0" { pos %r %r %r; color 1 0.95 0.9; power 9000 }' % LIGHTS[scene][0],
              'PointLight "l1" { pos %r %r %r; color 0.7 0.8 1; power 7000 }' % LIGHTS[scene][1]]
    textures = ['BitmapTexture "bmp" { file "floor.bmp"; scaling 0.05 }']
    shader_text = ['Lambert "sh_ground" { texture "bmp" }', 'Lambert "sh_a" { color 0.8 0.7 0.6 }',
                   'Phong "sh_b" { color 0.2 0.6 0.3; exponent 12; strength 0.5 }', 'Phong "sh_c" { color 0.7 0.5 0.2; exponent 16; strength 0 }',
                   'Lambert "sh_d" { color 0.3 0.4 0.8 }', 'Phong "sh_e" { color 0.6 0.2 0.5; exponent 40; strength 1 }']
    return "\n".join([
        "Scene {", '  Name "csg_edge_%s"' % scene,
        "  GlobalSettings { frameWidth %d; frameHeight %d; AAEnabled false; ambientLightColor 0.08 0.1 0.12 }" % (W, H),
        "  Camera { %s }" % CAMERA[scene],
        "  Lights {\n    " + "\n    ".join(lights) + "\n  }",
        "  Geometries {\n    " + "\n    ".join(geoms) + "\n  }",
        "  Textures {\n    " + "\n    ".join(textures) + "\n  }",
        "  Shaders {\n    " + "\n    ".join(shader_text) + "\n  }",
        "  Nodes {\n    " + "\n    ".join(nodes) + "\n  }",
        "}", ""])


class Case:
    """scene: the loaded scene (owns every table but the one replaced) | desc: the copied descriptor | cam, opts: the
    61x47 one-tap frame | nt: (n_nodes, 30) node_transform as the device gets it | geoms: per tree {letter: geometry id}"""


@functools.lru_cache(maxsize=None)
def load(name, tag=None):
    """`tag`: a loaded scene of the caller's own; None is the shared, read-only one"""
    path = os.path.join(_TMP, "csg_edge_%s%s.sdl" % (name, "_" + tag if tag else ""))
    with open(path, "w") as f:
        f.write(scene_text(name))
    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    scene.setAA(False)
    scene.setDof(False)
    src = scene.desc.contents
    assert src.n_nodes == 1 + len(TREES[name]) <= 28
    d = _abi.SceneDesc()
    C.memmove(C.byref(d), C.byref(src), C.sizeof(d))
    nt = np.array([src.node_transform[i] for i in range(30 * src.n_nodes)], dtype=np.float64).reshape(src.n_nodes, 30)
    lib = _abi.load_library()
    for i, t in enumerate(TREES[name]):
        if t[5] is not None:
            angles, scale, off = t[5]
            m = (C.c_double * 30)()
            lib.c2rt_host_transform_reset(m)
            lib.c2rt_host_transform_rotate(m, *angles)
            if scale:
                lib.c2rt_host_transform_scale(m, *scale)
            lib.c2rt_host_transform_translate(m, (C.c_double * 3)(*off))
            nt[i + 1] = list(m)
    assert np.array_equal(nt[GROUND, :9], np.eye(3).ravel()) and not nt[GROUND, 27:].any()
    if name == "identity":
        assert all(np.array_equal(r[:9], np.eye(3).ravel()) and not r[27:].any() for r in nt)
    flat = np.ascontiguousarray(nt.ravel())
    d.node_transform = flat.ctypes.data_as(type(d.node_transform))
    case = Case()
    case.name, case.scene, case.desc, case.nt, case._keep = name, scene, d, nt, flat
    case.cam = scene.beginFrame()
    case.opts = scene.renderOpts(taps=_abi.TAPS_1)
    case.geoms = scene_geom_names(name)
    return case


@functools.lru_cache(maxsize=None)
def scene_geom_names(scene):
    """per tree {letter: geometry id} in the order the text declares them (geometry 0 is the ground)"""
    out, g = [], 1
    for name, tree, centre, s, _, _ in TREES[scene]:
        lines, names = tree_text(name, tree, centre, s)
        ids = {}
        for k, line in enumerate(lines):
            gname = line.split('"')[1]
            for letter, n in names.items():
                if n == gname:
                    ids[letter] = g + k
        out.append(ids)
        g += len(lines)
    return out


def carved_box(scene, name):
    """world box (lo, hi) of what a depth-1 CsgDiff of two cubes of scene "identity" takes away as the camera sees it:
    a ∩ e where the two overlap (Diff(a, e)); the whole of b where they only share a face (Diff(a, b): a ∩ b has no
    volume, and b is the space through which that face is seen)"""
    _, tree, (X, Y, Z), s, _, _ = TREES[scene][node_index(scene, name) - 1]
    h = s // 2
    centre = {"a": (X, Y, Z), "b": (X - s, Y, Z), "e": (X, Y + 2 * (s // 5), Z)}
    l, r = np.array(centre[tree[1]], dtype=np.float64), np.array(centre[tree[2]], dtype=np.float64)
    lo, hi = np.maximum(l - h, r - h), np.minimum(l + h, r + h)
    return (lo, hi) if (hi > lo).all() else (r - h, r + h)


# ---- ray sets -------------------------------------------------------------------------------------------------------------


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)


def _tree_rays(rng, tree, centre, s, k):
    """object-space rays at one tree, (k-ish, 6), in chunks: [generic aimed rays | the rest].  Generic: origins on a
    sphere around the tree, aimed into it.  The rest: axis-parallel rays; origins and directions IN a shared plane
    (x = X +- h, y = Y +- h, z = Z +- h: whichever the tree's children share, the ray stays in it exactly because that
    component of the direction is 0); origins inside the solid and inside the carved part; origins ON a plane with a
    free direction."""
    Cc = np.array(centre, dtype=np.float64)
    h = s / 2.0
    n_gen = k // 2
    o = Cc + _unit(rng.normal(size=(n_gen, 3))) * 2.5 * s
    generic = np.hstack([o, _unit(Cc + rng.uniform(-0.45, 0.45, size=(n_gen, 3)) * s - o)])
    rest = []
    n_ax, n_pl, n_in, n_on = k // 8, k // 6, k // 8, k - n_gen - k // 8 - k // 6 - k // 8
    # axis-parallel
    ax = AXES[rng.randint(0, 6, size=n_ax)]
    q = Cc + rng.uniform(-0.48, 0.48, size=(n_ax, 3)) * s
    rest.append(np.hstack([q - ax * 2.0 * s, ax]))
    # in a face plane of `a`: origin on it, direction within it (half of them axis-parallel)
    for j in range(n_pl):
        axis = (0, 0, 1, 2)[j % 4]
        q = Cc + rng.uniform(-0.45, 0.45, size=3) * s
        q[axis] = Cc[axis] + (h if (j // 4) % 2 else -h)
        v = _unit(rng.normal(size=3))
        v[axis] = 0.0
        v = AXES[2 * ((axis + 1 + j % 2) % 3) + (j // 2) % 2].copy() if j % 3 == 0 else _unit(v)
        rest.append(np.hstack([q - v * rng.uniform(0.2, 2.0) * s, v])[None, :])
    # origins inside: the solid, the carved part (above / beside the centre), the spheres
    q = Cc + rng.uniform(-0.45, 0.45, size=(n_in, 3)) * s
    q[1::3, 1] += 0.4 * s
    q[2::3, 0] -= 0.6 * s
    rest.append(np.hstack([q, _unit(rng.normal(size=(n_in, 3)))]))
    # origins ON a plane of `a`, free direction
    for j in range(n_on):
        axis = j % 3
        q = Cc + rng.uniform(-0.45, 0.45, size=3) * s
        q[axis] = Cc[axis] + (h if (j // 3) % 2 else -h)
        rest.append(np.hstack([q, _unit(rng.normal(size=3))])[None, :])
    if tree[1:] == ("a", "b") and tree[0] == "I":          # IN the shared face plane x = X - h: the only rays that hit Inter(a, b)
        for j in range(48):
            q = Cc + rng.uniform(-0.45, 0.45, size=3) * s
            q[0] = Cc[0] - h
            v = _unit(rng.normal(size=3) * (0.0, 1.0, 1.0))
            rest.append(np.hstack([q - v * rng.uniform(0.2, 2.0) * s, v])[None, :])
    if tree[1] == tree[2]:                                  # Op(a, a): more origins inside a
        q = Cc + rng.uniform(-0.45, 0.45, size=(32, 3)) * s
        rest.append(np.hstack([q, _unit(rng.normal(size=(32, 3)))]))
    if "s" in str(tree):                                    # the depth-4 tree is what is left of a's lower slab
        o = Cc + _unit(rng.normal(size=(64, 3))) * 2.5 * s
        tgt = Cc + rng.uniform(-0.45, 0.45, size=(64, 3)) * s
        tgt[:, 1] = Cc[1] - 0.3 * s
        rest.append(np.hstack([o, _unit(tgt - o)]))
    return generic, np.vstack(rest)


def _cap_rays(rng, k):
    """along the cap tree's axis, both ways, a hair off it (a third of them exactly parallel to it)"""
    o, d, t0, _ = cap_axis()
    lo, hi = min(v[0] for v in CAP_SPHERES.values()), max(v[1] for v in CAP_SPHERES.values())
    out = np.zeros((k, 6))
    for j in range(k):
        sgn = 1.0 if j % 4 else -1.0
        start = o + d * (t0 + ((lo - 30) if sgn > 0 else (hi + 30)) * CAP_UNIT)
        side = np.cross(d, rng.normal(size=3))
        out[j, :3] = start + side / np.linalg.norm(side) * rng.uniform(0.0, 0.15)
        out[j, 3:] = sgn * d if j % 3 == 0 else _unit(sgn * d + rng.normal(scale=0.002, size=3))
    return out


def _to_world(nt_row, rays):
    """Transform.point / direction in plain numpy: where to aim, not under test"""
    m, off = nt_row[0:9].reshape(3, 3), nt_row[27:30]
    return np.hstack([rays[:, :3] @ m + off, rays[:, 3:] @ m])


def _base_eyeless(case, seed, n):
    rng = np.random.RandomState(seed)
    trees = TREES[case.name]
    per = min((n - 64 * GROUPS - 160) // len(trees), 190)
    generic, rest = {}, []
    for i, (name, tree, centre, s, _, _) in enumerate(trees):
        g, r = _tree_rays(rng, tree, centre, s, per - (60 if name == "cap" else 0))
        if name == "cap":
            r = np.vstack([r, _cap_rays(rng, 60)])
        generic[name] = _to_world(case.nt[i + 1], g)
        if name == "depth4":                    # from where the camera stands: what is left of the tree is a thin slab
            o = np.array([2.0, 64.0, -52.0]) + rng.normal(scale=6.0, size=(200, 3))
            tgt = case.nt[i + 1][27:30] + np.array([0.0, -5.0, 0.0]) + rng.uniform(-5.0, 5.0, size=(200, 3))
            rest.append(np.hstack([o, _unit(tgt - o)]))
        rest.append(_to_world(case.nt[i + 1], r))
    rest = np.vstack(rest)
    k = n - 64 * GROUPS - len(rest) - sum(len(g) for g in generic.values())
    o = np.array([0.0, 25.0, 20.0]) + rng.uniform(-1, 1, size=(k, 3)) * np.array([70.0, 30.0, 60.0])
    rest = np.vstack([rest, np.hstack([o, _unit(rng.normal(size=(k, 3)))])])
    return generic, rest


def _group_pool(case, tname, seed):
    """candidates for the ordered groups: rays aimed at one tree, and rays of the kinds that tie on it"""
    rng = np.random.RandomState(seed)
    i = node_index(case.name, tname) - 1
    _, tree, centre, s, _, _ = TREES[case.name][i]
    g, r = _tree_rays(rng, tree, centre, s, 1600)
    return _to_world(case.nt[i + 1], np.vstack([g, r]))


@functools.lru_cache(maxsize=None)
def eyeless_rays(name, seed=EYELESS_SEED, n=N_EYELESS):
    """About 2000 seeded rays that share no eye: per tree, in its object space and carried to the world with the node's
    matrix, the rays of _tree_rays; rays along the cap tree's axis; origins in the scene's box; lengths 0.5 and 3.

    The first GROUPS * 64 rays are ORDERED BY THE REFERENCE'S FLAGS (geom_reference.Trace.node_flags) for the two trees of
    GROUP_TREES: a 64-aligned group of 64 rays that all meet the tree (both children hit) with no tied, odd, long or
    capped list under it — the device's wave-wide regular case — then a group with exactly ONE ray with a tied or odd
    list among 63 such: the two sides of the `__all` of a wave.  (Lengths are left at 1 in these groups.)"""
    case = load(name)
    generic, rest = _base_eyeless(case, seed, n)
    T = gr.Tables(case.desc)
    groups = []
    for k, tname in enumerate(GROUP_TREES[name]):
        node = node_index(name, tname)
        pool = _group_pool(case, tname, seed + 1 + k)
        _, S = gr.trace(T, pool)
        odd = S.flag("tied_list", node) | S.flag("odd_list", node)
        irregular = odd | S.flag("long_list", node) | S.flag("capped_list", node)
        met = _meets_both_children(T, case.nt[node], scene_geom_names(name)[node - 1], pool)
        reg = np.nonzero(~irregular & met)[0]
        bad = np.nonzero(odd)[0]
        assert len(reg) >= 127 and len(bad) >= 1, (tname, len(reg), len(bad))
        groups += [pool[reg[:64]], np.vstack([pool[reg[64:64 + 37]], pool[bad[:1]], pool[reg[64 + 37:127]]])]
    body = list(generic.values()) + [rest]
    tail = np.vstack(body)
    tail[3::10, 3:] *= 0.5
    tail[7::10, 3:] *= 3.0
    rays = np.ascontiguousarray(np.vstack(groups + [tail]))
    rays.setflags(write=False)
    return rays


def _meets_both_children(T, nt_row, ids, rays):
    """slab test of the ray against the boxes of the tree's two cube children (plain numpy: a choice of rays)"""
    m_inv, off = nt_row[9:18].reshape(3, 3), nt_row[27:30]
    o, d = (rays[:, :3] - off) @ m_inv, rays[:, 3:] @ m_inv
    ok = np.ones(len(rays), dtype=bool)
    for g in set(ids.values()):
        if T.geom_type[g] != gr.GEOM_CUBE:
            continue
        c, h = T.geom_param[g, :3], T.geom_param[g, 3] * 0.5 - 1e-3
        with np.errstate(all="ignore"):
            t0, t1 = (c - h - o) / d, (c + h - o) / d
        lo, hi = np.nanmax(np.minimum(t0, t1), axis=1), np.nanmin(np.maximum(t0, t1), axis=1)
        ok &= (lo < hi) & (lo > 1e-3)
    return ok


@functools.lru_cache(maxsize=None)
def ray_set(scene, name):
    case = load(scene)
    if name == "screen":
        return screen_rays(case.cam, W, H)
    return eyeless_rays(scene)


# ---- the carved parts of Diff(a, e) and Diff(a, b) on the screen (scene "identity") --------------------------------------

CARVED = ("diff_ae", "diff_ab")


def seen_through(rays, recs, lo, hi):
    """rays that cross the open box (lo, hi) and whose record lies at or beyond the point where they leave it (or is a
    miss): what they show was seen THROUGH the box.  A slab test in plain numpy (a choice of pixels, not under test);
    the box is shrunk by 1e-3 and the distance compared with the same slack."""
    o, d = rays[:, :3], rays[:, 3:]
    with np.errstate(all="ignore"):
        t0, t1 = (lo + 1e-3 - o) / d, (hi - 1e-3 - o) / d
    enter, leave = np.nanmax(np.minimum(t0, t1), axis=1), np.nanmin(np.maximum(t0, t1), axis=1)
    return (enter < leave) & (leave > 0) & (recs["dist"] >= leave - 1e-3)


def tiles(mask):
    """(tiles wholly inside `mask`, tiles that `mask` cuts) over the frame's 8x8 tiles (partial ones at the edges count)"""
    m = mask.reshape(H, W)
    whole = cut = 0
    for y in range(0, H, 8):
        for x in range(0, W, 8):
            t = m[y:y + 8, x:x + 8]
            whole += bool(t.all())
            cut += bool(t.any() and not t.all())
    return whole, cut

"""Build-authored scene and seeded ray sets for tests/test_geom_reference.py (CPU) and tests/test_gpu_geom.py: the one
scene of the suite whose node matrices have off-diagonal entries.

The text goes through the host loader (which can only make diagonal matrices: it mirrors the reference's quirk that
`rotate` is a second `scale`, rt/node.d:89-90); the descriptor is then COPIED and given a node_transform table of the
test's own, and a finite Plane limit through geom_param.  Reads tests/golden/scenes/floor.bmp only.  Object scale ~10.

Nodes (table order) -> geometry:
   0 GROUND        Plane y = 0, identity, zero offset (keeps ground_node and the shadow rectangles alive)
   1 SLOPE         Plane under rotate(25, -55, 12): kNodePlaneNormal without kNodeAxisPlane, a world normal with three
                   non-zero components; a wall behind the objects
   2 LID           Plane with limit 38, identity + offset (-10, 40, 40): a finite patch ABOVE light 0
   3 ROT_CUBE      Cube under rotate(30, 20, 10); shades the ground from light 0
   4 ROT_SPHERE    Sphere under rotate(40, -25, 15) then scale(1.3, 0.7, 1.0) (what the reference's Transform API makes)
   5 SHEAR_CUBE    Cube (off-centre) under SHEAR, a matrix with M != M^T entry by entry
   6 SHEAR_SPHERE  Sphere (off-centre) under SHEAR_2; shades the ground from light 0
   7 UNION         CsgUnion(Cube, Sphere) under a rotation
   8 INTER         CsgInter(Cube, Sphere) under a rotation
   9 DIFF          CsgDiff(Cube, Sphere) under a rotation
  10 NESTED        CsgDiff(CsgUnion(CsgInter(Cube, Sphere), Sphere), Sphere) under a rotation: depth 3, the LEFT child is a
                   CsgOp at two levels (the leaf-identity quirk of `current.g is left`)
  11 DIFF_ID       CsgDiff(Cube, Sphere) under the identity (the void-tile cull runs beside the general nodes); the cube's
                   centre has x == z, so rays mirrored in x and z meet two face pairs at EQUAL distance
  12 SPHERE_ID     Sphere under the identity (the silhouette cull)
Rotations are made by c2rt_host_transform_rotate (all three angles non-zero).  The shears' inverses are computed in
np.longdouble (cofactors) and rounded; the transposed inverse is the exact transpose of that.

Lights: variant "L1" has light 0 only, below the LID; "L2" adds one to the right of the camera."""
import ctypes as C
import functools
import os
import shutil
import tempfile

import numpy as np

import chess2rt_amd as c2
from chess2rt_amd import _abi
from golden_configs import SCENES
from ray_query_util import screen_rays

W, H = 61, 47
VARIANTS = ("L1", "L2")
GROUND, SLOPE, LID, ROT_CUBE, ROT_SPHERE, SHEAR_CUBE, SHEAR_SPHERE, UNION, INTER, DIFF, NESTED, DIFF_ID, SPHERE_ID = range(13)
N_NODES = 13
GENERAL = (SLOPE, ROT_CUBE, ROT_SPHERE, SHEAR_CUBE, SHEAR_SPHERE, UNION, INTER, DIFF, NESTED)   # off-diagonal entries
DIFF_NODES = (DIFF, NESTED, DIFF_ID)
LID_GEOM, LID_LIMIT = 2, 38.0
LIGHT0, LIGHT1 = (-20.0, 32.0, 10.0), (45.0, 35.0, -30.0)
EYELESS_SEED, N_EYELESS = 29, 2000

SHEAR = np.array([[1.1, 0.35, -0.2], [-0.15, 0.8, 0.25], [0.3, -0.1, 1.3]])
SHEAR_2 = np.array([[0.9, -0.25, 0.3], [0.2, 1.2, -0.1], [-0.35, 0.15, 0.75]])

# node -> (ops, offset); ops: ("rotate", yaw, pitch, roll) | ("scale", x, y, z) | ("matrix", M)
PLACEMENT = {
    GROUND: ((), (0.0, 0.0, 0.0)),
    SLOPE: ((("rotate", 25.0, -55.0, 12.0),), (0.0, 0.0, 130.0)),
    LID: ((), (-10.0, 40.0, 40.0)),
    ROT_CUBE: ((("rotate", 30.0, 20.0, 10.0),), (-30.0, 13.0, -6.0)),
    ROT_SPHERE: ((("rotate", 40.0, -25.0, 15.0), ("scale", 1.3, 0.7, 1.0)), (-8.0, 22.0, 30.0)),
    SHEAR_CUBE: ((("matrix", SHEAR),), (28.0, 11.0, 8.0)),
    SHEAR_SPHERE: ((("matrix", SHEAR_2),), (-6.0, 9.0, -30.0)),
    UNION: ((("rotate", -20.0, 35.0, 50.0),), (-42.0, 24.0, 35.0)),
    INTER: ((("rotate", 15.0, -40.0, 25.0),), (42.0, 14.0, -2.0)),
    DIFF: ((("rotate", -35.0, 10.0, -20.0),), (14.0, 9.0, -40.0)),
    NESTED: ((("rotate", 25.0, 15.0, -30.0),), (2.0, 12.0, -14.0)),
    DIFF_ID: ((), (0.0, 0.0, 0.0)),
    SPHERE_ID: ((), (0.0, 0.0, 0.0)),
}

GEOMS = ['Plane "ground" { y 0 }', 'Plane "slope" { y 0 }', 'Plane "lid" { y 0 }',
         'Cube "rc" { center 0 0 0; side 12 }', 'Sphere "rs" { center 0 0 0; R 7.5 }',
         'Cube "sc" { center 1 -0.5 0.5; side 10 }', 'Sphere "ss" { center -0.5 1 0.5; R 6 }',
         'Cube "u_c" { center 0 0 0; side 9 }', 'Sphere "u_s" { center 4 3 -2; R 5.5 }', 'CsgUnion "union" { left "u_c"; right "u_s" }',
         'Cube "i_c" { center 0 0 0; side 11 }', 'Sphere "i_s" { center 1 1 -1; R 7 }', 'CsgInter "inter" { left "i_c"; right "i_s" }',
         'Cube "d_c" { center 0 0 0; side 12 }', 'Sphere "d_s" { center 3 4 -4; R 6.5 }', 'CsgDiff "diff" { left "d_c"; right "d_s" }',
         'Cube "n_c" { center 0 0 0; side 12 }', 'Sphere "n_s1" { center 0 0 0; R 7.5 }', 'CsgInter "n_i" { left "n_c"; right "n_s1" }',
         'Sphere "n_s2" { center 6 2 0; R 4 }', 'CsgUnion "n_u" { left "n_i"; right "n_s2" }',
         'Sphere "n_s3" { center 0 5 -5; R 5 }', 'CsgDiff "nested" { left "n_u"; right "n_s3" }',
         'Cube "k" { center 30 22 30; side 12 }', 'Sphere "ks" { center 30 26 24; R 6 }', 'CsgDiff "diff_id" { left "k"; right "ks" }',
         'Sphere "ball" { center 58 27 25; R 7.5 }']
NODE_GEOM_NAMES = ("ground", "slope", "lid", "rc", "rs", "sc", "ss", "union", "inter", "diff", "nested", "diff_id", "ball")
NODE_SHADERS = ("sh_ground", "sh_slope", "sh_lid", "sh_a", "sh_b", "sh_c", "sh_d", "sh_a", "sh_e", "sh_c", "sh_b", "sh_e", "sh_d")
TIE_CUBE = (np.array([30.0, 22.0, 30.0]), 12.0)       # "k": centre x == z

_TMP = tempfile.mkdtemp(prefix="c2rt_geom_")
shutil.copy(os.path.join(SCENES, "floor.bmp"), os.path.join(_TMP, "floor.bmp"))


def scene_text(variant):
    lights = ['PointLight "l0" { pos %r %r %r; color 1 0.95 0.9; power 1800 }' % LIGHT0]
    if variant == "L2":
        lights.append('PointLight "l1" { pos %r %r %r; color 0.7 0.8 1; power 2400 }' % LIGHT1)
    textures = ['BitmapTexture "bmp" { file "floor.bmp"; scaling 0.05 }', 'Checker "chk" { color1 0.9 0.1 0.2; color2 0.15 0.8 0.95; size 2.5 }']
    shaders = ['Lambert "sh_ground" { texture "bmp" }', 'Lambert "sh_slope" { texture "chk" }', 'Lambert "sh_lid" { color 0.6 0.6 0.7 }',
               'Lambert "sh_a" { color 0.8 0.7 0.6 }', 'Phong "sh_b" { color 0.2 0.6 0.3; exponent 12; strength 0.5 }',
               'Phong "sh_c" { color 0.7 0.5 0.2; exponent 16; strength 0 }', 'Lambert "sh_d" { color 0.3 0.4 0.8 }',
               'Phong "sh_e" { color 0.6 0.2 0.5; exponent 40; strength 1 }']
    nodes = ['Node "n%d" { geometry "%s"; shader "%s" }' % (i, g, s) for i, (g, s) in enumerate(zip(NODE_GEOM_NAMES, NODE_SHADERS))]
    return "\n".join([
        "Scene {", '  Name "geom_%s"' % variant,
        "  GlobalSettings { frameWidth %d; frameHeight %d; AAEnabled false; ambientLightColor 0.08 0.1 0.12 }" % (W, H),
        "  Camera { pos 5 24 -72; yaw 0; pitch -17; roll 0; fov 78 }",
        "  Lights {\n    " + "\n    ".join(lights) + "\n  }",
        "  Geometries {\n    " + "\n    ".join(GEOMS) + "\n  }",
        "  Textures {\n    " + "\n    ".join(textures) + "\n  }",
        "  Shaders {\n    " + "\n    ".join(shaders) + "\n  }",
        "  Nodes {\n    " + "\n    ".join(nodes) + "\n  }",
        "}", ""])


def inverse_longdouble(m):
    """the inverse of a 3x3 by cofactors in np.longdouble, rounded to double once"""
    a = np.asarray(m, dtype=np.longdouble)
    cof = np.empty((3, 3), dtype=np.longdouble)
    for i in range(3):
        for j in range(3):
            r, c = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            minor = a[r[0], c[0]] * a[r[1], c[1]] - a[r[0], c[1]] * a[r[1], c[0]]
            cof[i, j] = minor if (i + j) % 2 == 0 else -minor
    det = a[0, 0] * cof[0, 0] + a[0, 1] * cof[0, 1] + a[0, 2] * cof[0, 2]
    return (cof.T / det).astype(np.float64)


@functools.lru_cache(maxsize=None)
def node_transforms():
    """(N_NODES, 30) float64: transform, inverseTransform, transposedInverse, offset of every node"""
    lib = _abi.load_library()
    out = np.zeros((N_NODES, 30))
    for node, (ops, off) in PLACEMENT.items():
        t = (C.c_double * 30)()
        lib.c2rt_host_transform_reset(t)
        for op in ops:
            if op[0] == "rotate":
                lib.c2rt_host_transform_rotate(t, *op[1:])
            elif op[0] == "scale":
                lib.c2rt_host_transform_scale(t, *op[1:])
            else:
                inv = inverse_longdouble(op[1])
                t[0:9] = list(np.asarray(op[1], dtype=np.float64).ravel())
                t[9:18] = list(inv.ravel())
                t[18:27] = list(inv.T.ravel())
        lib.c2rt_host_transform_translate(t, (C.c_double * 3)(*off))
        out[node] = list(t)
    return out


class Case:
    """scene: the loaded scene (owns every table but the two replaced) | desc: the copied descriptor | cam, opts: the
    61x47 one-tap frame | cams: three cameras of an orbit (cams[0] is cam)"""


@functools.lru_cache(maxsize=None)
def load(variant, tag=None):
    """`tag`: a loaded scene of the caller's own (its camera and frame size may be set); None is the shared, read-only one"""
    path = os.path.join(_TMP, "geom_%s%s.sdl" % (variant, "_" + tag if tag else ""))
    with open(path, "w") as f:
        f.write(scene_text(variant))
    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    scene.setAA(False)
    scene.setDof(False)
    src = scene.desc.contents
    assert src.n_nodes == N_NODES and src.n_geoms == len(GEOMS)
    d = _abi.SceneDesc()
    C.memmove(C.byref(d), C.byref(src), C.sizeof(d))
    nt = np.ascontiguousarray(node_transforms().ravel())
    gp = np.array([src.geom_param[i] for i in range(4 * src.n_geoms)], dtype=np.float64)
    gp[4 * LID_GEOM + 1] = LID_LIMIT
    d.node_transform = nt.ctypes.data_as(type(d.node_transform))
    d.geom_param = gp.ctypes.data_as(type(d.geom_param))
    case = Case()
    case.scene, case.desc, case._keep = scene, d, (nt, gp)
    case.cam = scene.beginFrame()
    case.opts = scene.renderOpts(taps=_abi.TAPS_1)
    case.cams = [case.cam]
    for _ in range(2):
        scene.rotateCamera(7.0, 0, 0)
        case.cams.append(scene.beginFrame())
    scene.rotateCamera(-14.0, 0, 0)
    scene.beginFrame()
    return case


# ---- ray sets -------------------------------------------------------------------------------------------------------------


def _point(node, q):
    """Transform.point in plain numpy: where to aim, not under test"""
    t = node_transforms()[node]
    return np.asarray(q, dtype=np.float64) @ t[0:9].reshape(3, 3) + t[27:30]


def _leaves(case):
    """[(node, geometry type, centre, size)] of every Sphere / Cube leaf under every node"""
    d = case.desc
    out = []

    def walk(node, g):
        t = d.geom_type[g]
        if t in (_abi.GEOM_SPHERE, _abi.GEOM_CUBE):
            out.append((node, t, np.array([d.geom_param[4 * g + k] for k in range(3)]), d.geom_param[4 * g + 3]))
        elif t >= _abi.GEOM_CSG_UNION:
            walk(node, d.geom_child[2 * g])
            walk(node, d.geom_child[2 * g + 1])
    for n in range(d.n_nodes):
        walk(n, d.node_geom[n])
    return out


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)


def eyeless_rays(case, seed=EYELESS_SEED, n=N_EYELESS):
    """Rays that share no eye, built like ray_query_util.eyeless_rays but aimed with each node's WORLD placement
    (point() of the leaf centres): random origins in the scene's box, half of them aimed at a leaf; origins INSIDE
    solids and inside the cavities of the differences (the subtracted spheres' centres); the six axis directions in the
    world and in every general node's object space (direction() of the object axes: back in object space the other two
    components are zero only up to rounding); origins on a cube's face plane in object space; rays at the LID inside
    and outside its limit; rays mirrored in x and z at the vertical edges of DIFF_ID's cube (two face pairs at equal
    distance); lengths 0.5 and 3."""
    rng = np.random.RandomState(seed)
    leaves = _leaves(case)
    T = node_transforms()
    chunks = []

    def aimed(k, spread=2.0):
        pick = [leaves[i] for i in rng.randint(0, len(leaves), size=k)]
        return np.array([_point(nd, c) for nd, _, c, _ in pick]) + rng.normal(scale=spread, size=(k, 3))

    def box(k):
        return np.array([0.0, 25.0, 15.0]) + rng.uniform(-1, 1, size=(k, 3)) * np.array([75.0, 35.0, 85.0])

    # (a) axis directions in the world, towards leaves
    tgt = aimed(36, 1.0)
    v = np.tile(AXES, (6, 1))
    chunks.append(np.hstack([tgt - v * rng.uniform(15, 60, size=(36, 1)), v]))
    # (b) axis directions of every general node's object space, three rays each
    for node in GENERAL:
        m = T[node][0:9].reshape(3, 3)
        mine = [l for l in leaves if l[0] == node] or [(node, None, np.zeros(3), 20.0)]
        for a in AXES:
            for _ in range(3):
                _, _, c, size = mine[rng.randint(len(mine))]
                q = c + rng.uniform(-0.4, 0.4, size=3) * size
                wd = a @ m
                chunks.append(np.hstack([_point(node, q - a * rng.uniform(1.5, 4.0) * size), wd])[None, :])
    # (c) origins on a cube's face plane in object space
    cubes = [l for l in leaves if l[1] == _abi.GEOM_CUBE]
    for k in range(80):
        node, _, c, size = cubes[k % len(cubes)]
        q = c + rng.uniform(-0.45, 0.45, size=3) * size
        q[k % 3] = c[k % 3] + (0.5 if (k // 3) % 2 else -0.5) * size
        chunks.append(np.hstack([_point(node, q), _unit(rng.normal(size=3))])[None, :])
    # (d) origins inside solids and cavities
    o = aimed(260, 1.5)
    chunks.append(np.hstack([o, _unit(rng.normal(size=(260, 3)))]))
    # (e) the LID: inside and outside its limit, from below and from above
    off = np.array(PLACEMENT[LID][1])
    tgt = off + np.stack([rng.uniform(-60, 60, 150), np.zeros(150), rng.uniform(-60, 60, 150)], axis=1)
    o = box(150)
    o[::3, 1] = rng.uniform(45, 70, size=len(o[::3]))
    chunks.append(np.hstack([o, _unit(tgt - o)]))
    # (f) mirrored in x and z: both face pairs of cube "k" at the same distance
    c, side = TIE_CUBE
    ties = np.zeros((160, 6))
    for k in range(160):
        sx, sz = (1.0, -1.0)[k & 1], (1.0, -1.0)[(k >> 1) & 1]
        a = rng.uniform(2.0, 25.0)
        y = c[1] + rng.uniform(-0.45, 0.45) * side
        dy = rng.uniform(-0.05, 0.05)
        ties[k, :3] = (c[0] + sx * (0.5 * side + a), y, c[2] + sz * (0.5 * side + a))
        ties[k, 3:] = (-sx, dy, -sz)
        ties[k, 3:] /= np.sqrt(2.0 + dy * dy)
    chunks.append(ties)
    # (g) the rest: origins in the box, half aimed at a leaf
    rest = n - sum(len(c_) for c_ in chunks)
    o = box(rest)
    v = rng.normal(size=(rest, 3))
    aim = rng.rand(rest) < 0.5
    v = _unit(np.where(aim[:, None], aimed(rest) - o, v))
    chunks.append(np.hstack([o, v]))
    rays = np.ascontiguousarray(np.vstack(chunks))
    assert rays.shape == (n, 6)
    rays[3::10, 3:] *= 0.5
    rays[7::10, 3:] *= 3.0
    return rays


RAY_SETS = ("screen", "eyeless")


@functools.lru_cache(maxsize=None)
def ray_set(name):
    """the geometry is the same in both variants, so are the rays"""
    case = load("L1")
    if name == "screen":
        return screen_rays(case.cam, W, H)
    return eyeless_rays(case)

"""Scenes with CsgDiff(L, Sphere) nodes that the mask pre-pass may drop from tiles (chess2rt_amd/csrc/csg_void.h),
shared by the host tests (tests/test_csg_void_tiles.py) and the GPU tests (tests/test_gpu_csg_void.py), so that both
check the same scenes.  Every generator returns SDL text; every scene shades with Lambert only (the GPU frames are
bit-equal to the oracle's), except lecture5 itself."""
import math
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LECTURE5 = os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl")

CAMERA = "Camera {{ pos {pos}; yaw {yaw:.6g}; pitch {pitch:.6g}; roll {roll:.6g}; fov {fov:.6g} }}"


def cam(pos, yaw, pitch, roll=0.0, fov=90.0):
    return CAMERA.format(pos=" ".join("%.9g" % v for v in pos), yaw=yaw, pitch=pitch, roll=roll, fov=fov)


def left_geom(name, kind, c, half):
    """a Cube of side 2 half or a Sphere of radius half"""
    if kind == "Cube":
        return 'Cube "{0}" {{ center {1} {2} {3}; side {4:.9g} }}'.format(name, c[0], c[1], c[2], 2 * half)
    return 'Sphere "{0}" {{ center {1} {2} {3}; R {4:.9g} }}'.format(name, c[0], c[1], c[2], half)


def scene_text(camera, lights, geoms, nodes, floor_y=-0.01, aa=True, floor_at=0):
    """lights: [(x, y, z)]; geoms / nodes: SDL lines; a Plane "floor" at floor_y is geometry 0 and node `floor_at`"""
    nodes = list(nodes)
    nodes.insert(floor_at, 'Node "floor" { geometry "floor"; shader "sh" }')
    lt = "\n".join('    PointLight "l%d" { pos %.9g %.9g %.9g; color 1 1 1; power 800000 }' % (i, p[0], p[1], p[2])
                   for i, p in enumerate(lights))
    return """Scene {{
  GlobalSettings {{ frameWidth 64; frameHeight 48; ambientLightColor 0.2 0.2 0.2; AAEnabled {aa} }}
  {cam}
  Lights {{
{lights}
  }}
  Geometries {{
    Plane "floor" {{ y {fy:.9g} }}
{geoms}
  }}
  Shaders {{
    Lambert "sh" {{ color 0.5 0.5 0.5 }}
    Lambert "sh2" {{ color 0.2 0.6 0.3 }}
  }}
  Nodes {{
{nodes}
  }}
}}
""".format(aa="true" if aa else "false", cam=camera, lights=lt, fy=floor_y, geoms="\n".join("    " + g for g in geoms),
           nodes="\n".join("    " + n for n in nodes))


def diff_scene(left_kind, c, half, R, camera, light, off=(0, 0, 0), lights=None, floor_y=-0.01):
    """Diff(Cube | Sphere "L", Sphere "S") as node 1 (translated by `off`) over the floor (node 0); light 0 = light"""
    geoms = [left_geom("L", left_kind, c, half),
             'Sphere "S" {{ center {0} {1} {2}; R {3:.17g} }}'.format(c[0], c[1], c[2], R),
             'CsgDiff "D" { left "L"; right "S" }']
    nodes = ['Node "d" {{ geometry "D"; shader "sh"; translate {0} {1} {2} }}'.format(*off)]
    return scene_text(camera, [light] + list(lights or []), geoms, nodes, floor_y=floor_y)


def fuzz_scene(seed):
    """The fuzzed Diff(Cube | Sphere, Sphere) scenes: random box, sphere from barely touching the left child to
    swallowing it, random camera aimed near it (roll, fov), random light, a translation half of the time."""
    r = random.Random(1000 + seed)
    kind = r.choice(["Cube", "Sphere"])
    c = (r.uniform(-60, 60), r.uniform(20, 80), r.uniform(80, 260))
    half = r.uniform(10, 60)
    R = half * (r.uniform(1.0, 1.8) if kind == "Cube" else r.uniform(0.6, 1.6))
    target = (c[0] + r.uniform(-30, 30), c[1] + r.uniform(-30, 30), c[2] + r.uniform(-30, 30))
    pos = (r.uniform(-200, 200), r.uniform(5, 300), r.uniform(-150, 80))
    d = [target[i] - pos[i] for i in range(3)]
    yaw = math.degrees(math.atan2(d[0], d[2])) + r.uniform(-15, 15)
    pitch = math.degrees(math.atan2(d[1], math.hypot(d[0], d[2]))) + r.uniform(-10, 10)
    light = (r.uniform(-300, 300), r.uniform(150, 800), r.uniform(-100, 500))
    off = (r.uniform(-20, 20), r.uniform(0, 20), r.uniform(-20, 20)) if r.random() < 0.5 else (0, 0, 0)
    return diff_scene(kind, c, half, R, cam(pos, yaw, pitch, r.uniform(-20, 20), r.uniform(30, 100)), light, off)


def lecture5_like(R, pos, yaw=0.0, pitch=-30.0, light=(-90, 700, 350), off=(0, 0, 0), lights=None):
    """lecture5's CSG object (cube of side 100 at (-100, 60, 200) minus a sphere of radius R) alone over the floor"""
    return diff_scene("Cube", (-100, 60, 200), 50, R, cam(pos, yaw, pitch), light, off, lights)


# ---- adversarial set-ups: (name, sdl), rendered at 160x120 ------------------------------------------------------

def just_large_enough():
    # half-diagonal of the cube face: 50 * sqrt(2) ~ 70.71 — edges poke out below it, vanish above it
    return [("big%g" % R, lecture5_like(R, (0, 165, 0))) for R in (70.7106, 70.7107, 70.71068, 86.6025, 86.6026, 90.0)]


def tangent_rays():
    # the sphere tangent to the cube's faces (R = half side) and the eye level with the top face
    return [("tan%g_%g_%g" % (R, pos[0], pos[1]), lecture5_like(R, pos, pitch=0.0 if pos[1] == 110 else -10.0))
            for R, pos in ((50.0, (0, 110, 0)), (50.0, (-100, 110, 0)), (50.000001, (-100, 60, 0)), (70.0, (-100, 110, -40)))]


def eye_inside():
    # inside the sphere but outside the box, inside both, inside the box near a corner (outside the sphere)
    return [("in%g_%g" % (pos[0], pos[2]), lecture5_like(70.0, pos, yaw, pitch))
            for pos, yaw, pitch in (((-100, 60, 135), 0.0, 0.0), ((-100, 60, 200), 30.0, -20.0), ((-140, 100, 160), 45.0, 10.0))]


def light_inside_box():
    return [("light_in", lecture5_like(70.0, (0, 165, 0), light=(-100, 60, 200)))]


def adversarial():
    return just_large_enough() + tangent_rays() + eye_inside() + light_inside_box()


# ---- set-ups for branches lecture5 never takes ------------------------------------------------------------------

def light_below_ground(granted):
    """The ground is a ceiling (y = 200) above the box, light 0 below it: the h < 0 branch of the shadow flag.
    granted: the light under the box (y = -100), flag bit 1 set; else the light at the box's mid height, refused."""
    ly = -100.0 if granted else 60.0
    return diff_scene("Cube", (-100, 60, 200), 50, 70.0, cam((-60, -20, 40), -15.0, 40.0), (-120, ly, 230), floor_y=200.0)


def several_lights(n):
    """lecture5's object seen from close by, light 0 as in lecture5 (shadow-void tiles in front of the box) and n - 1
    further lights; light 1, low behind the box, casts the node's shadow forward onto some of those tiles."""
    extra = [(-100, 90, 700), (250, 400, -50), (-400, 300, 100)][: n - 1]
    return lecture5_like(70.0, (-100, 160, 60), 0.0, -35.0, light=(-90, 700, 350), lights=extra)


def _diff_block(tag, kind, c, half, R, right_kind="Sphere"):
    return [left_geom("L" + tag, kind, c, half),
            ('Sphere "S{0}" {{ center {1} {2} {3}; R {4:.9g} }}' if right_kind == "Sphere" else
             'Cube "S{0}" {{ center {1} {2} {3}; side {4:.9g} }}').format(tag, c[0], c[1], c[2], R),
            'CsgDiff "D{0}" {{ left "L{0}"; right "S{0}" }}'.format(tag)]


def several_candidates(n_cand):
    """n_cand CsgDiff(Cube, Sphere) candidates in a row (the library tests the first four), mixed with CsgDiff nodes
    that are no candidates: rotated, scaled, Diff(Sphere, Cube) and Diff(L, L)."""
    geoms, nodes = [], []
    for k in range(n_cand):
        geoms += _diff_block("c%d" % k, "Cube" if k % 2 == 0 else "Sphere", (0, 60, 0), 50 if k % 2 == 0 else 55, 70.0)
    geoms += _diff_block("x", "Cube", (0, 30, 0), 25, 34.0)
    geoms += _diff_block("y", "Sphere", (0, 30, 0), 28, 40.0, right_kind="Cube")
    geoms += [left_geom("Lz", "Cube", (0, 30, 0), 25), 'CsgDiff "Dz" { left "Lz"; right "Lz" }']
    xs = [-260 + 130 * k for k in range(n_cand)]
    # non-candidates first and in between: rotated, Diff(Sphere, Cube), scaled, Diff(L, L)
    nodes.append('Node "rot" { geometry "Dx"; shader "sh2"; rotate 0 30 0; translate -300 0 420 }')
    for k, x in enumerate(xs):
        nodes.append('Node "c{0}" {{ geometry "Dc{0}"; shader "sh"; translate {1} 0 {2} }}'.format(k, x, 200 + 30 * (k % 2)))
        if k == 1:
            nodes.append('Node "sc" { geometry "Dy"; shader "sh2"; translate 0 0 520 }')
    nodes.append('Node "scl" { geometry "Dx"; shader "sh2"; scale 1.2 1.2 1.2; translate 260 0 500 }')
    nodes.append('Node "ll" { geometry "Dz"; shader "sh2"; translate -150 0 560 }')
    return scene_text(cam((0, 160, 60), 0.0, -35.0), [(-50, 800, 300)], geoms, nodes)


def candidates_at_0_31_33():
    """candidates at node indices 0, 31 and 33 (the floor is node 1, small spheres fill the rest): the library tests
    nodes below kMaxCullNodes = 32 only, and with more than 32 nodes no ground refinement runs."""
    geoms = _diff_block("a", "Cube", (0, 60, 0), 50, 70.0) + ['Sphere "f" { center 0 0 0; R 3 }']
    nodes = []
    for n in range(35):  # + the floor at index 1: nodes 0..35
        k = n + 1 if n >= 1 else n
        if k in (0, 31, 33):
            x = {0: -130, 31: 0, 33: 130}[k]
            nodes.append('Node "n{0}" {{ geometry "Da"; shader "sh"; translate {1} 0 200 }}'.format(k, x))
        else:
            nodes.append('Node "n{0}" {{ geometry "f"; shader "sh2"; translate {1} 3 {2} }}'.format(k, -300 + 17 * k, 120 + 5 * k))
    return scene_text(cam((0, 160, 60), 0.0, -35.0), [(-50, 800, 300)], geoms, nodes, floor_at=1)


def translated_candidate():
    return lecture5_like(70.0, (-62.5, 172.25, 19), 0.0, -35.0, off=(37.5, 12.25, -41.0))


def camera_path():
    """rotateCamera / moveCamera steps from lecture5's camera (0, 165, 0), yaw 0, pitch -30 (a move runs along the
    camera's right, up and front directions as the last frame left them; the level camera's are +x, +y, +z), each
    followed by a frame: level, into the sphere outside the box (-100, 60, 135), into both (-100, 60, 200), looking around there, into the box's
    corner outside the sphere (-145, 105, 155), looking around, and back out.  [(dyaw, droll, dpitch, dx, dy, dz)]"""
    return [(0, 0, 30, 0, 0, 0), (0, 0, 0, -100, -105, 135), (0, 0, 0, 0, 0, 65), (25, 0, -10, 0, 0, 0),
            (-25, 0, 10, 0, 0, 0), (0, 0, 0, -45, 45, -45), (40, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, -150)]

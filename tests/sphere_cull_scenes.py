"""Scenes of Sphere nodes over a floor that the mask pre-pass may drop from tiles outside their silhouette
(chess2rt_amd/csrc/csg_void.h: cone_misses_ball), shared by tests/test_sphere_cull_tiles.py and
tests/test_gpu_sphere_cull.py.  Every generator returns SDL text (Lambert only, as tests/csg_void_scenes.py)."""
import math
import random

import csg_void_scenes as S

LECTURE5 = S.LECTURE5


def spheres_scene(balls, camera, light, floor_y=-0.01, offs=None):
    """balls: [(cx, cy, cz, R)] as nodes 1.. over the floor (node 0); offs: per-ball translation or None"""
    geoms = ['Sphere "s%d" { center %.17g %.17g %.17g; R %.17g }' % ((k,) + tuple(b)) for k, b in enumerate(balls)]
    nodes = []
    for k in range(len(balls)):
        tr = "" if not offs or offs[k] is None else "; translate %.9g %.9g %.9g" % tuple(offs[k])
        nodes.append('Node "n%d" { geometry "s%d"; shader "%s"%s }' % (k, k, "sh" if k % 2 else "sh2", tr))
    return S.scene_text(camera, [light], geoms, nodes, floor_y=floor_y)


def fuzz_scene(seed):
    """1-5 random balls (the library tests the first four), random camera aimed near the first (roll, fov), random
    light — sometimes lower than a ball's top —, a translated ball half of the time"""
    r = random.Random(7000 + seed)
    n = r.randint(1, 5)
    balls = [(r.uniform(-150, 150), r.uniform(5, 120), r.uniform(60, 400), r.uniform(5, 60)) for _ in range(n)]
    offs = [(r.uniform(-30, 30), r.uniform(0, 30), r.uniform(-30, 30)) if r.random() < 0.5 else None for _ in range(n)]
    c = balls[0]
    target = (c[0] + r.uniform(-40, 40), c[1] + r.uniform(-40, 40), c[2] + r.uniform(-40, 40))
    pos = (r.uniform(-250, 250), r.uniform(5, 300), r.uniform(-200, 50))
    d = [target[i] - pos[i] for i in range(3)]
    yaw = math.degrees(math.atan2(d[0], d[2])) + r.uniform(-15, 15)
    pitch = math.degrees(math.atan2(d[1], math.hypot(d[0], d[2]))) + r.uniform(-10, 10)
    light = (r.uniform(-300, 300), r.uniform(60, 800), r.uniform(-100, 500))
    return spheres_scene(balls, S.cam(pos, yaw, pitch, r.uniform(-20, 20), r.uniform(30, 110)), light, offs=offs)


def adversarial():
    """[(name, sdl)]: set-ups where the test must refuse or be right"""
    rp = 30.0
    out = []
    # the eye inside the ball, and just inside / outside the padded ball (the margin is ~4e-4 here)
    for name, z in (("eye_inside", 100.0), ("eye_in_pad", 100.0 - 30.0 - 1e-4), ("eye_outside", 100.0 - 30.0 - 1e-2)):
        out.append((name, spheres_scene([(0, 50, 100, rp)], S.cam((0, 50, z), 0.0, -20.0), (-90, 700, 350))))
    # a ball behind the eye (and one in front)
    out.append(("behind", spheres_scene([(0, 60, -80, 40), (30, 40, 200, 25)], S.cam((0, 80, 0), 0.0, -25.0), (-90, 700, 350))))
    # a field of view of nearly 180 degrees
    out.append(("fov179", spheres_scene([(0, 40, 120, 35), (-90, 20, 60, 20)], S.cam((0, 90, 0), 0.0, -30.0, 0.0, 179.0), (-90, 700, 350))))
    # the light below the ball's top, and level with its centre
    out.append(("light_low", spheres_scene([(0, 60, 200, 50), (120, 20, 160, 20)], S.cam((0, 165, 0), 0.0, -30.0), (-150, 100, 150))))
    out.append(("light_level", spheres_scene([(0, 60, 200, 50)], S.cam((0, 165, 0), 0.0, -30.0), (-250, 60, 200))))
    # a ball that straddles the ground
    out.append(("straddle", spheres_scene([(0, 5, 200, 40), (-120, 30, 260, 30)], S.cam((0, 165, 0), 0.0, -30.0), (-90, 700, 350))))
    # coordinates of 1e6
    o = 1.0e6
    out.append(("far1e6", spheres_scene([(o, 60, o + 200, 50), (o - 120, 30, o + 260, 30)], S.cam((o, 165, o), 0.0, -30.0),
                                        (o - 90, 700, o + 350))))
    # a translated ball
    out.append(("translated", spheres_scene([(0, 0, 0, 45)], S.cam((0, 165, 0), 0.0, -30.0), (-90, 700, 350), offs=[(-40, 50, 220)])))
    return out

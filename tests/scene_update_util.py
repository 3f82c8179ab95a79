"""Shared by the scene-update tests (tests/test_scene_update_plan.py on the CPU, tests/test_gpu_scene_update.py and
tests/test_gpu_frames_posed.py on the GPU): descriptions patched in Python — the yardstick of every case is a fresh
plan / a fresh upload of such a description, never the update under test — transforms built with the host mirror's
Transform, the scenes and the sequences of poses both sides run."""
import ctypes as C
import os

import numpy as np

import chess2rt_amd as c2
import scene_fuzz
from chess2rt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")

# c2rt_scene_desc tables: field -> (count field, elements per entry, dtype)
_TABLES = {
    "geom_type": ("n_geoms", 1, np.int32), "geom_param": ("n_geoms", 4, np.float64), "geom_child": ("n_geoms", 2, np.int32),
    "tex_type": ("n_textures", 1, np.int32), "tex_color": ("n_textures", 18, np.float32), "tex_param": ("n_textures", 6, np.float64),
    "tex_scaling": ("n_textures", 1, np.float32), "tex_width": ("n_textures", 1, np.uint32), "tex_height": ("n_textures", 1, np.uint32),
    "tex_offset": ("n_textures", 1, np.uint64), "texels": ("n_texels", 3, np.float32),
    "shader_type": ("n_shaders", 1, np.int32), "shader_color": ("n_shaders", 3, np.float32), "shader_texture": ("n_shaders", 1, np.int32),
    "shader_exponent": ("n_shaders", 1, np.float64), "shader_strength": ("n_shaders", 1, np.float32),
    "light_type": ("n_lights", 1, np.int32), "light_pos": ("n_lights", 3, np.float64), "light_color": ("n_lights", 3, np.float32),
    "light_power": ("n_lights", 1, np.float32),
    "node_geom": ("n_nodes", 1, np.int32), "node_shader": ("n_nodes", 1, np.int32), "node_bump": ("n_nodes", 1, np.int32),
    "node_transform": ("n_nodes", 30, np.float64),
}


class Desc:
    """A deep copy of a c2rt_scene_desc in numpy arrays: .d is the SceneDesc over them, .a[field] the arrays."""

    def __init__(self, desc):
        src = desc.contents if hasattr(desc, "contents") else desc
        self.d = _abi.SceneDesc.from_buffer_copy(src)
        self.a = {}
        # a pointer field keeps no reference to the array it was set from: .d owns the arrays, so that
        # Desc(...).d and base.patched(...).d stay valid after the Desc itself is gone
        self.d._arrays = self.a
        for field, (count, per, dtype) in _TABLES.items():
            n = int(getattr(src, count)) * per
            ptr = getattr(src, field)
            arr = np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n and ptr else np.zeros(max(n, 1), dtype=dtype)
            self.a[field] = arr
            setattr(self.d, field, arr.ctypes.data_as(type(getattr(self.d, field))))

    def patched(self, nodes=None, lights=None):
        """a new Desc with nodes = {index: transform30} and lights = {index: dict(pos=, color=, power=)} written in"""
        out = Desc(self.d)
        for n, t in (nodes or {}).items():
            out.a["node_transform"][30 * n:30 * n + 30] = np.asarray(t, dtype=np.float64).reshape(30)
        for l, v in (lights or {}).items():
            if "pos" in v:
                out.a["light_pos"][3 * l:3 * l + 3] = v["pos"]
            if "color" in v:
                out.a["light_color"][3 * l:3 * l + 3] = np.asarray(v["color"], dtype=np.float32)
            if "power" in v:
                out.a["light_power"][l] = np.float32(v["power"])
        return out

    def transform(self, n):
        return self.a["node_transform"][30 * n:30 * n + 30].copy()


# ---- Transform (rt/transform.d) through the host mirror: the bits a D caller would hand over ----
def xf(*steps):
    """reset, then the steps in order: ("scale", x, y, z) | ("translate", x, y, z) | ("rotate", yaw, pitch, roll)"""
    lib = _abi.load_library()
    t = np.empty(30, dtype=np.float64)
    p = t.ctypes.data_as(_abi._f64p)
    lib.c2rt_host_transform_reset(p)
    for step in steps:
        if step[0] == "scale":
            lib.c2rt_host_transform_scale(p, *[float(v) for v in step[1:]])
        elif step[0] == "rotate":
            lib.c2rt_host_transform_rotate(p, *[float(v) for v in step[1:]])
        elif step[0] == "translate":
            lib.c2rt_host_transform_translate(p, (C.c_double * 3)(*[float(v) for v in step[1:]]))
        else:
            raise ValueError(step)
    return t


def xf_with(index, value):
    """the identity with one of its 30 doubles replaced (a NaN, an infinity)"""
    t = xf()
    t[index] = value
    return t


# ---- scenes ----
def _scene_text(lights, geoms, nodes, shaders=None):
    lt = "\n".join('    PointLight "l%d" { pos %.9g %.9g %.9g; color 1 1 1; power %g }' % (i, p[0], p[1], p[2], w)
                   for i, (p, w) in enumerate(lights))
    return """Scene {
  GlobalSettings { frameWidth 96; frameHeight 64; ambientLightColor 0.2 0.2 0.2; AAEnabled false }
  Camera { pos 0 165 0; yaw 0; pitch -30; roll 0; fov 90 }
  Lights {
%s
  }
  Geometries {
%s
  }
  Shaders {
    Lambert "sh" { color 0.5 0.5 0.5 }
    Lambert "sh2" { color 0.2 0.6 0.3 }
    Phong "ph" { color 0.1 0.2 0.7; exponent 40 }
  }
  Nodes {
%s
  }
}
""" % (lt, "\n".join("    " + g for g in geoms), "\n".join("    " + n for n in nodes))


LIGHT0 = ((-90, 700, 350), 800000)


def lecture5_like(n_lights=1):
    """lecture5's layout without its bitmaps: node 0 the floor (y -0.01), node 1 a sphere, node 2 Diff(cube, sphere),
    nodes 3..5 a small sphere translated three ways; light 0 lecture5's, lights 1 and 2 elsewhere"""
    lights = [LIGHT0, ((200, 400, -50), 300000), ((0, 300, 500), 200000)][:n_lights]
    geoms = ['Plane "floor" { y -0.01 }', 'Sphere "globe" { center 100 50 320; R 50 }',
             'Cube "cube" { center -100 60 200; side 100 }', 'Sphere "hole" { center -100 60 200; R 70 }',
             'CsgDiff "diff" { left "cube"; right "hole" }', 'Sphere "S" { R 15 }']
    nodes = ['Node "floor" { geometry "floor"; shader "sh" }', 'Node "globe" { geometry "globe"; shader "sh2" }',
             'Node "csg" { geometry "diff"; shader "ph" }',
             'Node "S1" { geometry "S"; shader "ph"; translate 100 15 256 }',
             'Node "S2" { geometry "S"; shader "ph"; translate 50 15 206 }',
             'Node "S3" { geometry "S"; shader "ph"; translate 0 15 156 }']
    return _scene_text(lights, geoms, nodes)


def planes_only():
    """two axis planes, one light: the plane instances"""
    geoms = ['Plane "floor" { y -0.01 }', 'Plane "shelf" { y 40 }']
    nodes = ['Node "floor" { geometry "floor"; shader "sh" }', 'Node "shelf" { geometry "shelf"; shader "sh2" }']
    return _scene_text([LIGHT0], geoms, nodes)


def nested_csg():
    """a depth-2 CsgOp over the floor: the hit-stack retry launch (csg_stress.sdl's kind, small)"""
    geoms = ['Plane "floor" { y -0.01 }', 'Cube "c" { center 0 60 220; side 100 }', 'Sphere "s" { center 0 60 220; R 65 }',
             'Sphere "t" { center 30 90 180; R 40 }', 'CsgInter "cs" { left "c"; right "s" }', 'CsgDiff "top" { left "cs"; right "t" }',
             'Sphere "ball" { center -120 30 200; R 30 }']
    nodes = ['Node "floor" { geometry "floor"; shader "sh" }', 'Node "obj" { geometry "top"; shader "ph" }',
             'Node "ball" { geometry "ball"; shader "sh2" }']
    return _scene_text([LIGHT0], geoms, nodes)


def load_text(tmp_path, text, name, size=(96, 64)):
    import shutil

    shutil.copy(os.path.join(SCENES, "floor.bmp"), str(tmp_path / "floor.bmp"))
    p = tmp_path / name
    p.write_text(text)
    scene = c2.parseSceneFromFile(str(p))
    scene.setFrameSize(*size)
    scene.setAA(False)
    return scene


def forty_nodes(tmp_path):
    """a ground plane and 39 objects: node 31 is the last the culling masks cover, 32.. are always tested"""
    scene = load_text(tmp_path, scene_fuzz.many_nodes_scene_sdl(1, 39), "forty.sdl")
    assert scene.desc.contents.n_nodes == 40
    return scene


# ---- the sequences of poses, each a list of (nodes, lights) applied one after the other ----
def sequences():
    """{case: (scene key, [(nodes, lights), ...])}; scene keys: l5 (lecture5_like, one light), l5x3 (three lights),
    planes, forty"""
    nan, inf = float("nan"), float("inf")
    return {
        # 1: identity -> translated -> scaled -> back to identity, on the sphere node 1
        "sphere_moves": ("l5", [({1: xf(("translate", -30, 10, -40))}, None), ({1: xf(("scale", 1.5, 0.75, 1.25))}, None), ({1: xf()}, None)]),
        # 2: the ground plane raised, then given a scale (and a general one: no axis plane any more), then back
        "ground_l5": ("l5", [({0: xf(("translate", 0, 5, 0))}, None), ({0: xf(("scale", 2, 3, 2))}, None), ({0: xf()}, None)]),
        "ground_planes": ("planes", [({0: xf(("translate", 0, 5, 0))}, None), ({0: xf(("scale", 2, 3, 2))}, None),
                                     ({1: xf(("rotate", 0, 20, 0))}, None), ({0: xf(), 1: xf()}, None)]),
        # 3: the CsgDiff node translated, and back
        "csg_translated": ("l5", [({2: xf(("translate", 40, 0, -30))}, None), ({2: xf()}, None)]),
        # 4: light 0 sideways, below the ground plane, onto its height; light 2 of three
        "light0": ("l5", [(None, {0: dict(pos=(150, 700, 100))}), (None, {0: dict(pos=(-90, -50, 350))}),
                          (None, {0: dict(pos=(-90, -0.01, 350))}), (None, {0: dict(pos=(-90, 700, 350))})]),
        "light2_of_three": ("l5x3", [(None, {2: dict(pos=(-200, 350, 100))}), (None, {0: dict(pos=(10, 600, 300))})]),
        # 5: power 0 and back, a colour of 2^70
        "light_values": ("l5", [(None, {0: dict(power=0.0)}), (None, {0: dict(power=800000.0)}),
                                (None, {0: dict(color=(2.0 ** 70, 1.0, 1.0), power=1.0)}), (None, {0: dict(color=(1, 1, 1), power=800000.0)})]),
        # 6: a NaN, an infinity, then finite again
        "nan_inf": ("l5", [({3: xf_with(4, nan)}, None), ({3: xf_with(28, inf)}, None), ({3: xf(("translate", 100, 15, 256))}, None)]),
        # 7: both sides of the 32-node width of the culling masks
        "forty": ("forty", [({31: xf(("translate", 5, 2, -3))}, None), ({32: xf(("scale", 1.25, 1.25, 1.25))}, None),
                            ({39: xf(("translate", -4, 1, 6)), 31: xf()}, None)]),
    }


def load_case_scene(key, tmp_path):
    if key == "l5":
        return load_text(tmp_path, lecture5_like(1), "l5.sdl")
    if key == "l5x3":
        return load_text(tmp_path, lecture5_like(3), "l5x3.sdl")
    if key == "planes":
        return load_text(tmp_path, planes_only(), "planes.sdl")
    if key == "forty":
        return forty_nodes(tmp_path)
    raise KeyError(key)

"""Scenes for tests/test_csg_tile_plan.py (CPU) and tests/test_gpu_csg_tiles.py: lecture5.sdl with its text edited (the
CsgOp's material, the floor's texture, the light, the node order) and its CsgOp rewritten in the descriptor (operator,
children, the node's matrix) — the kinds of leaf trees tests/csg_edge_scenes.py holds (the three operators, cube and
sphere in both orders, cubes that share a face plane), in a scene that fits lean::csg_tile's condition: one light, the
ground and the CsgOp node alone in some tiles.  (csg_edge_scenes.py's own scenes have two lights and 18 nodes: no tile of
theirs is eligible.)"""
import os

from chess2rt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")

CUBE = [0, -100.0, 60.0, 200.0, 100.0]
SPHERE = [1, -100.0, 60.0, 200.0, 70.0]
PAIRS = {"cs": (CUBE, SPHERE), "sc": (SPHERE, CUBE), "ss": ([1, -100.0, 60.0, 200.0, 60.0], [1, -60.0, 80.0, 170.0, 50.0]),
         "cc_shared_face": ([0, -100.0, 60.0, 200.0, 100.0], [0, 0.0, 60.0, 200.0, 100.0])}

_CSG_SHADER = 'Phong {\n      name      "csg_shader"\n      color     0.5 0.5 0\n      exponent  60\n    }'
_FLOOR_SHADER = 'Lambert {\n      name    "floor_shader"\n      texture "bmp"\n    }'
_CSG_NODE = '    // CSG object:\n    Node {\n      name      "csgNode"\n      geometry  "diff"\n      shader    "csg_shader"\n    }\n'
_FLOOR_NODE = '    // Floor:\n    Node {\n      name      "floor"\n      geometry  "floor"\n      shader    "floor_shader"\n    }\n'
_CHECKER = '    Checker {\n      name "chk"\n      color1 0.9 0.9 0.9\n      color2 0.1 0.3 0.1\n      size 37\n    }\n'


def text(edit=None):
    """lecture5.sdl, edited: lambert (the CsgOp's material), checker / plain (the floor), light_below, light_low (a long
    shadow of the CsgOp on the floor and on itself), power_0, two_lights, csg_first (the CsgOp node in front of the
    floor in file order), csg_textured"""
    t = open(os.path.join(SCENES, "lecture5.sdl")).read()
    for e in (edit or "").split("+"):
        if e == "lambert":
            t = _replace(t, _CSG_SHADER, 'Lambert {\n      name      "csg_shader"\n      color     0.5 0.5 0\n    }')
        elif e == "checker":
            t = _replace(t, "  Textures {\n", "  Textures {\n" + _CHECKER)
            t = _replace(t, _FLOOR_SHADER, 'Lambert {\n      name    "floor_shader"\n      texture "chk"\n    }')
        elif e == "plain":
            t = _replace(t, _FLOOR_SHADER, 'Lambert {\n      name    "floor_shader"\n      color   0.6 0.7 0.5\n    }')
        elif e == "light_below":
            t = _replace(t, "pos    -90 700 350", "pos    -90 -300 350")
        elif e == "light_low":
            t = _replace(t, "pos    -90 700 350", "pos    -400 150 60")
        elif e == "power_0":
            t = _replace(t, "power  800000", "power  0")
        elif e == "two_lights":
            i = t.index("PointLight")
            j = t.index("}", i) + 1
            t = t[:j] + "\n    " + t[i:j].replace("light1", "light2").replace("-90 700 350", "150 500 100") + t[j:]
        elif e == "csg_first":
            t = _replace(t, _CSG_NODE, "")
            t = _replace(t, _FLOOR_NODE, _CSG_NODE + "\n" + _FLOOR_NODE)
        elif e == "csg_textured":
            t = _replace(t, _CSG_NODE, _CSG_NODE.replace('"csg_shader"', '"globe_shader"'))
        elif e:
            raise ValueError(e)
    return t


def _replace(t, old, new):
    assert t.count(old) == 1, old
    return t.replace(old, new)


def csg_node(d):
    """(node, geometry) of the scene's CsgOp"""
    return next((n, d.node_geom[n]) for n in range(d.n_nodes) if d.geom_type[d.node_geom[n]] >= _abi.GEOM_CSG_UNION)


def rewrite(scene, case):
    """the descriptor edits of a case: op, pair (PAIRS), translate, rotate, inel = plane | nested, no_light"""
    if case.get("translate"):
        scene.translateNode("csgNode", case["translate"])
    if case.get("rotate"):
        r = case["rotate"]
        scene.rotateNode("csgNode", r[0], r[1], r[2])
    d = scene.desc.contents
    _, g = csg_node(d)
    d.geom_type[g] = case.get("op", 5)
    l, r = d.geom_child[2 * g], d.geom_child[2 * g + 1]
    for c, k in zip((l, r), PAIRS[case.get("pair", "cs")]):
        d.geom_type[c] = _abi.GEOM_SPHERE if k[0] else _abi.GEOM_CUBE
        for i in range(4):
            d.geom_param[4 * c + i] = k[1 + i]
    if case.get("inel") == "plane":
        d.geom_type[r] = _abi.GEOM_PLANE
        for i, v in enumerate((60.0, float("nan"), 0.0, 0.0)):
            d.geom_param[4 * r + i] = v
    elif case.get("inel") == "nested":
        others = [k for k in range(d.n_geoms) if k not in (g, l, r) and d.geom_type[k] in (_abi.GEOM_SPHERE, _abi.GEOM_CUBE)]
        d.geom_type[r] = _abi.GEOM_CSG_UNION
        d.geom_child[2 * r], d.geom_child[2 * r + 1] = others[0], others[1]
    if case.get("no_light"):
        d.n_lights = 0

"""The planner that ships (chess2rt_amd/csrc/scene_plan.cpp, through its host build tests/libscene_plan_check.so)
against the Python restatements (scripts/csg_void_tiles.py, scripts/sphere_cull_tiles.py), on the CPU: the candidates,
the ground, and each frame's VoidCull and SphereCull bit for bit — what tests/csg_void_device.py and
tests/sphere_cull_device.py assert of the library on the GPU — and every refusal of plan_scene with its status and
message, leaving the plan it was given untouched.  These are host decisions, not pixels: two small frame sizes."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import chess2rt_amd as c2  # noqa: E402
import csg_void_scenes as V  # noqa: E402
import csg_void_tiles as cv  # noqa: E402
import scene_fuzz  # noqa: E402
import sphere_cull_scenes as S  # noqa: E402
import sphere_cull_tiles as sc  # noqa: E402
from chess2rt_amd import _abi  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
MAX_CSG_GEOMS = 4096  # include/c2rt.h
SIZES = ((64, 48), (320, 240))
DEBUG_CULLS = (0, 1, 2, 4, 8)
MASKS = (0, 1, 3)


class VoidNodeC(C.Structure):  # csg_void.h
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("c", C.c_double * 3), ("r2", C.c_double),
                ("node", C.c_uint32), ("flags", C.c_uint32)]


class VoidCullC(C.Structure):
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("light0", C.c_double * 3), ("v", VoidNodeC * cv.MAX_VOID_NODES)]


class SphereNodeC(C.Structure):
    _fields_ = [("c", C.c_double * 3), ("rp", C.c_double), ("node", C.c_uint32), ("flags", C.c_uint32)]


class SphereCullC(C.Structure):
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("reach", C.c_double), ("s", SphereNodeC * sc.MAX_SPHERE_NODES)]


class PlanFacts(C.Structure):  # tests/scene_plan_check.cpp
    _fields_ = [("ground_node", C.c_int32), ("csg_levels", C.c_int32), ("ground_y", C.c_double),
                ("planes_only", C.c_uint32), ("all_identity", C.c_uint32), ("n_nodes", C.c_uint32), ("n_lights", C.c_uint32),
                ("n_void", C.c_uint32), ("n_sphere", C.c_uint32), ("tables_hash", C.c_uint64),
                ("void_nodes", VoidNodeC * cv.MAX_VOID_NODES), ("sphere_nodes", SphereNodeC * sc.MAX_SPHERE_NODES)]


class FramePlan(C.Structure):
    _fields_ = [("n_cull", C.c_uint32), ("n_cull_lights", C.c_uint32), ("ground_node", C.c_int32),
                ("row_group_start", C.c_uint32), ("force_exact", C.c_uint32), ("pad", C.c_uint32),
                ("cull_rect", C.c_int32 * 4 * cv.MAX_CULL_NODES), ("cull_hull", C.c_float * 3 * 6 * cv.MAX_CULL_NODES),
                ("light_side", C.c_int32 * 8 * cv.MAX_CULL_LIGHTS), ("v", VoidCullC), ("s", SphereCullC)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(os.path.join(ROOT, "tests", "libscene_plan_check.so"))
        L.c2rt_plan_new.restype = C.c_void_p
        L.c2rt_plan_free.argtypes = [C.c_void_p]
        L.c2rt_plan_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        L.c2rt_plan_facts.argtypes = [C.c_void_p, C.POINTER(PlanFacts), C.c_void_p, C.c_size_t]
        L.c2rt_plan_facts.restype = C.c_size_t
        L.c2rt_plan_frame.argtypes = [C.c_void_p, C.POINTER(_abi.CameraFrame), C.POINTER(_abi.RenderOpts), C.c_int, C.c_uint32,
                                      C.c_uint32, C.POINTER(FramePlan), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        L.c2rt_plan_frame.restype = C.c_size_t
        _lib = L
    return _lib


class Plan:
    def __init__(self):
        self.h = C.c_void_p(lib().c2rt_plan_new())

    def __del__(self):
        lib().c2rt_plan_free(self.h)

    def plan(self, desc):
        msg = C.create_string_buffer(512)
        st = lib().c2rt_plan_scene(self.h, C.cast(desc, C.c_void_p) if desc is not None else None, msg, len(msg))
        return st, msg.value.decode()

    def facts(self):
        f = PlanFacts()
        boxed = (C.c_uint8 * 65536)()
        assert lib().c2rt_plan_facts(self.h, C.byref(f), boxed, len(boxed)) == C.sizeof(PlanFacts)  # one layout on both sides
        return f, bytes(boxed[: f.n_nodes])

    def frame(self, cam, opts, debug_cull=0, void_mask=3, sphere_mask=3):
        out, st, msg = FramePlan(), C.c_int(-1), C.create_string_buffer(512)
        assert lib().c2rt_plan_frame(self.h, C.byref(cam), C.byref(opts), debug_cull, void_mask, sphere_mask, C.byref(out),
                                     C.byref(st), msg, len(msg)) == C.sizeof(FramePlan)
        assert st.value == _abi.OK, msg.value
        return out


def _copy_cam(cam):
    out = _abi.CameraFrame()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(out))
    return out


def _moved_to(cam, pos):
    """the same view from another eye point"""
    out = _copy_cam(cam)
    d = [pos[i] - cam.pos[i] for i in range(3)]
    for name in ("pos", "up_left", "up_right", "down_left"):
        for i in range(3):
            getattr(out, name)[i] = getattr(cam, name)[i] + d[i]
    return out


def _cameras(scene, desc, inside=None):
    """[(name, camera)]: the scene's own; one with the eye inside the first candidate's box (`inside`: given, for
    lecture5 the camera of tests/test_gpu_frame_batch.py's walk); one with depth of field"""
    own = scene.beginFrame()
    cams = [("own", own)]
    if inside is None:
        cands = cv.void_candidates(desc)
        balls = sc.sphere_candidates(desc)
        if cands:
            inside = _moved_to(own, [0.5 * (cands[0].lo[i] + cands[0].hi[i]) for i in range(3)])
        elif balls:
            inside = _moved_to(own, balls[0].c)
    if inside is not None:
        cams.append(("inside", inside))
    dof = _copy_cam(own)
    dof.dof, dof.num_samples, dof.focal_plane_dist, dof.disc_multiplier = 1, 4, 100.0, 1.0
    cams.append(("dof", dof))
    return cams


def _void_entry(v):
    return dict(node=v.node, lo=list(v.lo), hi=list(v.hi), c=list(v.c), r2=v.r2, flags=v.flags)


def _check_scene(scene, inside=None):
    """the assertions of csg_void_device.compare / sphere_cull_device.compare that concern the host, on the planner"""
    desc = scene.desc
    D = cv._fields(desc)
    plan = Plan()
    st, msg = plan.plan(desc)
    assert st == _abi.OK, msg
    facts, boxed = plan.facts()
    # the scene: ground and candidates
    gn, gy = cv.ground_of(desc)
    if D.n_lights == 0:
        gn = None  # (the library keeps a ground only where light 0 exists: RenderParams::ground_node)
    assert facts.ground_node == (gn if gn is not None else -1)
    if gn is not None:
        assert facts.ground_y == gy
    cands, balls = cv.void_candidates(desc), sc.sphere_candidates(desc)
    assert [dict(node=v.node, lo=list(v.lo), hi=list(v.hi), c=list(v.c), R=v.r2, flags=v.flags) for v in facts.void_nodes[: facts.n_void]] == \
        [dict(node=c.node, lo=c.lo, hi=c.hi, c=c.c, R=c.R, flags=c.flags) for c in cands]
    assert [dict(node=s.node, c=list(s.c), R=s.rp, flags=s.flags) for s in facts.sphere_nodes[: facts.n_sphere]] == \
        [dict(node=b.node, c=b.c, R=b.R, flags=b.flags) for b in balls]
    for c in list(cands) + list(balls):
        assert boxed[c.node] == 1
    assert (facts.n_nodes, facts.n_lights) == (D.n_nodes, D.n_lights)
    last_boxed = max([n + 1 for n in range(min(D.n_nodes, cv.MAX_CULL_NODES)) if boxed[n]], default=0)
    # the frames
    n_checked = 0
    for W, H in SIZES:
        scene.setFrameSize(W, H)
        opts = scene.renderOpts()
        for cname, cam in _cameras(scene, desc, inside):
            for dc in DEBUG_CULLS:
                for mask in MASKS:
                    f = plan.frame(cam, opts, dc, mask, mask)
                    what = (cname, W, H, dc, mask)
                    if cname == "dof":
                        assert f.n_cull == 0 and f.v.n == 0 and f.s.n == 0, what
                        continue
                    assert f.n_cull == (0 if dc & 1 else last_boxed), what
                    assert f.ground_node == (-1 if dc & 2 or gn is None else gn), what
                    assert f.n_cull_lights == (0 if dc & 4 or not last_boxed else min(D.n_lights, cv.MAX_CULL_LIGHTS)), what  # (bit 0 clears n_cull alone)
                    assert f.force_exact == 0, what
                    want = cv.frame_void_nodes(desc, cam, dc)
                    want = [] if want is None else want
                    assert [_void_entry(f.v.v[j]) for j in range(f.v.n)] == [dict(w, flags=w["flags"] & mask) for w in want], what
                    assert list(f.v.light0) == ([D.light_pos[i] for i in range(3)] if D.n_lights else [0.0] * 3), what
                    swant = sc.frame_sphere_cull(desc, cam, dc, mask)
                    reach, entries = (0.0, []) if swant is None else swant
                    assert f.s.n == len(entries) and (f.s.reach == reach or not entries), what + (f.s.n, f.s.reach, swant)
                    for j, e in enumerate(entries):
                        s = f.s.s[j]
                        assert dict(node=s.node, c=list(s.c), rp=s.rp, flags=s.flags) == e, what + (j,)
                    n_checked += 1
    return facts, n_checked


def _from_text(tmp_path, text, name):
    import shutil

    shutil.copy(os.path.join(SCENES, "floor.bmp"), str(tmp_path / "floor.bmp"))
    p = tmp_path / (name + ".sdl")
    p.write_text(text)
    return c2.parseSceneFromFile(str(p))


def test_lecture5_and_csg_stress():
    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    # the third camera of tests/test_gpu_frame_batch.py's walk: the eye walked into the CSG object's box
    walker = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    walker.setFrameSize(72, 100)
    for rot, mov in (((0, 0, 0), (0, 0, 0)), ((-25, 0, 0), (0, 0, 100)), ((0, 0, 0), (0, 0, 120))):
        walker.rotateCamera(*rot)
        walker.beginFrame()
        walker.moveCamera(*mov)
        inside = walker.beginFrame()
    facts, n = _check_scene(scene, inside)
    # a corner of that box lies behind this eye: the node's rectangle is the whole frame, its hull unused
    plan = Plan()
    assert plan.plan(scene.desc)[0] == _abi.OK
    node = cv.void_candidates(scene.desc)[0].node
    scene.setFrameSize(64, 48)
    f = plan.frame(inside, scene.renderOpts())
    assert list(f.cull_rect[node]) == [-2**31, -2**31, 2**31 - 1, 2**31 - 1]
    assert [list(e) for e in f.cull_hull[node]] == [[0.0, 0.0, 1.0]] * 6
    own = plan.frame(scene.beginFrame(), scene.renderOpts())
    r = list(own.cull_rect[node])  # the file's camera sees the whole box in front of it: a finite rectangle
    assert -10**6 < r[0] < r[2] < 10**6 and -10**6 < r[1] < r[3] < 10**6
    assert (facts.n_void, facts.n_sphere, facts.csg_levels, facts.all_identity, facts.planes_only) == (1, 4, 1, 1, 0)
    assert n == 2 * 2 * len(DEBUG_CULLS) * len(MASKS)
    facts, _ = _check_scene(c2.parseSceneFromFile(os.path.join(SCENES, "csg_stress.sdl")))
    assert facts.csg_levels == 4


def _void_generators():
    g = [("fuzz%d" % s, V.fuzz_scene(s)) for s in range(8)] + V.adversarial()
    g += [("below_granted", V.light_below_ground(True)), ("below_refused", V.light_below_ground(False))]
    g += [("lights%d" % n, V.several_lights(n)) for n in (2, 3, 4)]
    g += [("cand%d" % n, V.several_candidates(n)) for n in (2, 4, 5)]
    g += [("cand_0_31_33", V.candidates_at_0_31_33()), ("translated", V.translated_candidate())]
    return g


def test_void_scene_generators(tmp_path):
    seen = {}
    for name, text in _void_generators():
        facts, _ = _check_scene(_from_text(tmp_path, text, name))
        seen[name] = facts.n_void
    assert seen["cand5"] == cv.MAX_VOID_NODES and seen["cand_0_31_33"] == 2 and seen["below_granted"] == 1


def test_sphere_scene_generators(tmp_path):
    total = 0
    for name, text in [("fuzz%d" % s, S.fuzz_scene(s)) for s in range(8)] + S.adversarial():
        facts, _ = _check_scene(_from_text(tmp_path, text, "s_" + name))
        total += facts.n_sphere
    assert total > 16


def test_fuzzed_scenes(tmp_path):
    """40 seeds of the general scene fuzzer (random transforms, nested CSG, several lights): mostly scenes whose nodes
    are NOT candidates, for reasons the restatements must share with the planner"""
    levels = set()
    for seed in range(40):
        facts, _ = _check_scene(_from_text(tmp_path, scene_fuzz.random_scene_sdl(seed), "f%d" % seed))
        levels.add(facts.csg_levels)
    assert len(levels) >= 3


# ---- refusals ---------------------------------------------------------------------------------------------------

_I = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]


class Tables:
    """a small valid scene as Python lists (a ground plane, a sphere, a Union of both kinds and a chain of Unions;
    a checker and a bitmap texture; one light; two nodes), turned into a SceneDesc on demand"""

    def __init__(self):
        self.abi_version, self.gi_enabled = _abi.ABI_VERSION, 0
        self.geom_type = [_abi.GEOM_PLANE, _abi.GEOM_SPHERE]
        self.geom_param = [0.0, 1e9, 0, 0, 0.0, 50.0, 100.0, 20.0]
        self.geom_child = [-1, -1, -1, -1]
        self.tex_type = [_abi.TEX_CHECKER, _abi.TEX_BITMAP]
        self.tex_width, self.tex_height, self.tex_offset = [0, 2], [0, 2], [0, 0]
        self.n_texels = 4
        self.shader_type = [_abi.SHADER_LAMBERT, _abi.SHADER_PHONG]
        self.shader_texture = [0, 1]
        self.light_type = [_abi.LIGHT_POINT]
        self.node_geom, self.node_shader = [0, 1], [0, 1]
        self.null = ()

    def add_geom(self, t, l=-1, r=-1):
        self.geom_type.append(t)
        self.geom_param += [0.0, 0.0, 0.0, 1.0]
        self.geom_child += [l, r]
        return len(self.geom_type) - 1

    def desc(self):
        keep = []

        def arr(ct, vals):
            a = (ct * max(len(vals), 1))(*vals)
            keep.append(a)
            return a

        ng, nt, ns, nl, nn = len(self.geom_type), len(self.tex_type), len(self.shader_type), len(self.light_type), len(self.node_geom)
        d = _abi.SceneDesc()
        d.abi_version, d.gi_enabled, d.max_trace_depth = self.abi_version, self.gi_enabled, 4
        d.n_geoms, d.n_textures, d.n_texels, d.n_shaders, d.n_lights, d.n_nodes = ng, nt, self.n_texels, ns, nl, nn
        tables = dict(
            geom_type=arr(C.c_int32, self.geom_type), geom_param=arr(C.c_double, self.geom_param), geom_child=arr(C.c_int32, self.geom_child),
            tex_type=arr(C.c_int32, self.tex_type), tex_color=arr(C.c_float, [0.5] * 18 * nt), tex_param=arr(C.c_double, [1.0] * 6 * nt),
            tex_scaling=arr(C.c_float, [1.0] * nt), tex_width=arr(C.c_uint32, self.tex_width), tex_height=arr(C.c_uint32, self.tex_height),
            tex_offset=arr(C.c_uint64, self.tex_offset), texels=arr(C.c_float, [0.25] * 3 * self.n_texels),
            shader_type=arr(C.c_int32, self.shader_type), shader_color=arr(C.c_float, [1.0] * 3 * ns),
            shader_texture=arr(C.c_int32, self.shader_texture), shader_exponent=arr(C.c_double, [8.0] * ns),
            shader_strength=arr(C.c_float, [1.0] * ns), light_type=arr(C.c_int32, self.light_type),
            light_pos=arr(C.c_double, [-90.0, 700.0, 350.0] * nl), light_color=arr(C.c_float, [1.0] * 3 * nl),
            light_power=arr(C.c_float, [5e5] * nl), node_geom=arr(C.c_int32, self.node_geom), node_shader=arr(C.c_int32, self.node_shader),
            node_bump=arr(C.c_int32, [-1] * nn), node_transform=arr(C.c_double, (_I * 3 + [0.0, 0.0, 0.0]) * nn))
        for name, a in tables.items():
            if name not in self.null:
                setattr(d, name, C.cast(a, type(getattr(d, name))))
        d._keep = keep
        return d


def _refusals():
    def case(status, message, edit):
        t = Tables()
        edit(t)
        return status, message, t

    def unknown_geom(t): t.geom_type[1] = 99
    def unknown_tex(t): t.tex_type[0] = 7
    def unknown_shader(t): t.shader_type[1] = 9
    def unknown_light(t): t.light_type[0] = 3
    def shader_index(t): t.node_shader[1] = 5
    def texture_index(t): t.shader_texture[0] = 2
    def cyclic(t): t.node_geom[1] = t.add_geom(_abi.GEOM_CSG_UNION, 2, 1)
    def geom_index(t): t.node_geom[1] = 17

    def too_deep(t):
        g = 1
        for _ in range(_abi.MAX_CSG_DEPTH + 1):
            g = t.add_geom(_abi.GEOM_CSG_UNION, g, 0)
        t.node_geom[1] = g

    def too_many(t):
        t.node_geom[1] = t.add_geom(_abi.GEOM_CSG_DIFF, 1, 0)
        while len(t.geom_type) <= MAX_CSG_GEOMS:
            t.add_geom(_abi.GEOM_SPHERE)

    def texels(t): t.tex_offset[1] = 1
    def null_table(t): t.null = ("shader_strength",)
    def null_texels(t): t.null = ("texels",)
    def gi(t): t.gi_enabled = 1
    def abi(t): t.abi_version = 7

    return {
        "unknown_geometry": case(_abi.ERR_UNSUPPORTED, "geometry 1: unknown type 99", unknown_geom),
        "unknown_texture": case(_abi.ERR_UNSUPPORTED, "texture 0: unknown type 7", unknown_tex),
        "unknown_shader": case(_abi.ERR_UNSUPPORTED, "shader 1: unknown type 9", unknown_shader),
        "unknown_light": case(_abi.ERR_UNSUPPORTED, "light 0: unknown type 3", unknown_light),
        "shader_index": case(_abi.ERR_INVALID_ARG, "node 1: shader index 5 out of range", shader_index),
        "texture_index": case(_abi.ERR_INVALID_ARG, "shader 0: texture index 2 out of range", texture_index),
        "cyclic_csg": case(_abi.ERR_INVALID_ARG, "node 1: geometry index out of range or cyclic CSG", cyclic),
        "geometry_index": case(_abi.ERR_INVALID_ARG, "node 1: geometry index out of range or cyclic CSG", geom_index),
        "too_deep": case(_abi.ERR_LIMIT, "node 1: CSG nesting 5 > 4", too_deep),
        "too_many_csg_geoms": case(_abi.ERR_LIMIT, "4097 geometries in a scene with CsgOps (limit 4096)", too_many),
        "texels_out_of_pool": case(_abi.ERR_INVALID_ARG, "texture 1: texels out of the pool", texels),
        "null_table": case(_abi.ERR_INVALID_ARG, "null table with non-zero count", null_table),
        "null_texels": case(_abi.ERR_INVALID_ARG, "null table with non-zero count", null_texels),
        "gi_enabled": case(_abi.ERR_UNSUPPORTED, "GIEnabled scenes (path tracing) are outside the hot path", gi),
        "abi_version": case(_abi.ERR_INVALID_ARG, "scene abi_version 7 != 1", abi),
    }


def _snapshot(plan):
    f, boxed = plan.facts()
    return bytes(f), boxed


def test_the_hand_built_scene_is_accepted():
    plan = Plan()
    t = Tables()
    t.node_geom[1] = t.add_geom(_abi.GEOM_CSG_DIFF, 1, 0)  # (and a scene at the geometry limit, with a CsgOp)
    while len(t.geom_type) < MAX_CSG_GEOMS:
        t.add_geom(_abi.GEOM_SPHERE)
    d = t.desc()
    assert plan.plan(C.pointer(d)) == (_abi.OK, "")
    f, boxed = plan.facts()
    assert (f.n_nodes, f.csg_levels, f.ground_node, f.ground_y, boxed) == (2, 1, 0, 0.0, b"\x00\x01")


@pytest.mark.parametrize("name", sorted(_refusals()))
def test_refusal_keeps_status_message_and_plan(name):
    """the statuses and messages are those c2rt_upload_scene has always given (chess2rt_amd/csrc/scene_plan.cpp holds
    the moved checks); the plan passed in still holds the scene planned before, table for table"""
    status, message, tables = _refusals()[name]
    plan = Plan()
    good = Tables().desc()
    assert plan.plan(C.pointer(good)) == (_abi.OK, "")
    before = _snapshot(plan)
    bad = tables.desc()
    assert plan.plan(C.pointer(bad)) == (status, message)
    assert _snapshot(plan) == before


def test_null_scene_is_refused():
    plan = Plan()
    assert plan.plan(None) == (_abi.ERR_INVALID_ARG, "null scene")

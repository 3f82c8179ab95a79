"""The pose-and-replan step behind c2rt_update_scene and c2rt_render_frames_posed, on the CPU, through
tests/libscene_update_check.so (tests/scene_update_check.cpp + chess2rt_amd/csrc/scene_plan.cpp, built without ROCm): the
helper drives scene_plan.cpp's own SceneCopy / update_scene_plan, the code the library runs.  The contract is equality
with a fresh upload: after every update of every sequence the whole ScenePlan — every table byte for byte, every scalar
fact — equals plan_scene of the description patched in Python.  These are the tests that catch a stale plan fact, which
GPU frames can hide behind the exactness of culling."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import scene_update_util as U
from chess2rt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 32 << 20

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(os.path.join(ROOT, "tests", "libscene_update_check.so"))
        L.c2rt_upd_new.restype = C.c_void_p
        L.c2rt_upd_new.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        L.c2rt_upd_free.argtypes = [C.c_void_p]
        L.c2rt_upd_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        L.c2rt_upd_plan_bytes.restype = C.c_size_t
        L.c2rt_upd_plan_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.c2rt_upd_fresh_plan_bytes.restype = C.c_size_t
        L.c2rt_upd_fresh_plan_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.c2rt_upd_frame_plan_bytes.restype = C.c_size_t
        L.c2rt_upd_frame_plan_bytes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
        _lib = L
    return _lib


_buf = None


def _take(call):
    global _buf
    if _buf is None:
        _buf = C.create_string_buffer(CAP)
    n = call(_buf, CAP)
    assert n <= CAP
    return bytes(_buf.raw[:n])


def sections(blob):
    """{name: bytes} of a serialised ScenePlan (tests/scene_update_check.cpp: 8-byte name, 8-byte size, bytes)"""
    out, at = {}, 0
    while at < len(blob):
        name = blob[at:at + 8].rstrip(b"\0").decode()
        (size,) = struct.unpack_from("<Q", blob, at + 8)
        out[name] = blob[at + 16:at + 16 + size]
        at += 16 + size
    return out


def scalar(sec, name, fmt):
    return struct.unpack("<" + fmt, sec[name])[0]


class Uploaded:
    def __init__(self, desc):
        st, msg = C.c_int(-1), C.create_string_buffer(512)
        self.h = lib().c2rt_upd_new(C.addressof(desc), C.byref(st), msg, len(msg))
        assert st.value == _abi.OK and self.h, msg.value

    def __del__(self):
        if getattr(self, "h", None):
            lib().c2rt_upd_free(self.h)

    def apply(self, pose):
        msg = C.create_string_buffer(512)
        st = lib().c2rt_upd_apply(self.h, C.addressof(pose) if pose is not None else None, msg, len(msg))
        return st, msg.value.decode()

    def plan(self):
        return _take(lambda b, n: lib().c2rt_upd_plan_bytes(self.h, b, n))

    def frame_plan(self, pose):
        st, msg = C.c_int(-1), C.create_string_buffer(512)
        blob = _take(lambda b, n: lib().c2rt_upd_frame_plan_bytes(self.h, C.addressof(pose), C.byref(st), msg, len(msg), b, n))
        assert st.value == _abi.OK, msg.value
        return blob


def fresh_plan(desc):
    st, msg = C.c_int(-1), C.create_string_buffer(512)
    blob = _take(lambda b, n: lib().c2rt_upd_fresh_plan_bytes(C.addressof(desc), C.byref(st), msg, len(msg), b, n))
    assert st.value == _abi.OK, msg.value
    return blob


def assert_same_plan(got, want, what):
    g, w = sections(got), sections(want)
    assert list(g) == list(w)
    for name in w:
        assert g[name] == w[name], "%s: plan section %r differs from the fresh plan's" % (what, name)
    assert got == want


SEQUENCES = U.sequences()


def _run(case, tmp_path):
    """[(facts after update k)], every one checked against the fresh plan of the patched description"""
    key, seq = SEQUENCES[case]
    scene = U.load_case_scene(key, tmp_path)
    cur = U.Desc(scene.desc)
    up = Uploaded(cur.d)
    assert_same_plan(up.plan(), fresh_plan(cur.d), case + " upload")
    facts = [sections(up.plan())]
    for k, (nodes, lights) in enumerate(seq):
        # a frame of a posed batch plans the same pose without keeping it: everything but texels4 equals the fresh plan
        nxt = cur.patched(nodes, lights)
        want = fresh_plan(nxt.d)
        before = up.plan()
        frame = sections(up.frame_plan(c2.makePose(nodes, lights)))
        for name, data in sections(want).items():
            assert frame[name] == (b"" if name == "texels4" else data), "%s frame %d: %r" % (case, k, name)
        assert up.plan() == before, "planning a posed frame changed the scene"
        st, msg = up.apply(c2.makePose(nodes, lights))
        assert st == _abi.OK, msg
        assert_same_plan(up.plan(), want, "%s update %d" % (case, k))
        facts.append(sections(want))
        cur = nxt
    return facts


import chess2rt_amd as c2  # noqa: E402


def _nodes_in(sec, name, size, node_at):
    data = sec[name]
    return [struct.unpack_from("<I", data, i * size + node_at)[0] for i in range(len(data) // size)]


def sphere_nodes(sec):
    return _nodes_in(sec, "spheres", 40, 32)


def void_nodes(sec):
    return _nodes_in(sec, "voids", 88, 80)


def test_sphere_moved_scaled_and_back(tmp_path):
    f = _run("sphere_moves", tmp_path)
    assert [scalar(s, "ident", "I") for s in f] == [1, 1, 0, 1]  # translations keep the identity matrix, the scale does not
    assert [1 in sphere_nodes(s) for s in f] == [True, True, False, True]
    assert f[0]["nodes"] != f[1]["nodes"] and f[0] == f[3]
    assert f[0]["rects"] != f[1]["rects"]


def test_ground_plane_raised_and_scaled(tmp_path):
    f = _run("ground_l5", tmp_path)
    assert [scalar(s, "ground", "i") for s in f] == [0, -1, -1, 0]  # the ground is a plane with zero offset and identity matrix
    assert scalar(f[0], "groundy", "d") == -0.01
    assert f[0] == f[3]


def test_planes_only_scene_loses_and_regains_its_instance(tmp_path):
    f = _run("ground_planes", tmp_path)
    # translated and axis-scaled planes stay axis planes; the rotated one does not
    assert [scalar(s, "planes", "I") for s in f] == [1, 1, 1, 0, 1]
    assert [scalar(s, "ident", "I") for s in f] == [1, 1, 0, 0, 1]
    assert [scalar(s, "ground", "i") for s in f] == [0, 1, 1, -1, 0]  # node 1 is the first plane left with zero offset


def test_csg_node_translated(tmp_path):
    f = _run("csg_translated", tmp_path)
    assert [void_nodes(s) for s in f] == [[2], [2], [2]]
    assert f[0]["voids"] != f[1]["voids"] and f[0]["box"] != f[1]["box"] and f[0] == f[2]


def test_light0_moves(tmp_path):
    f = _run("light0", tmp_path)
    assert len({s["lpos"] for s in f[:4]}) == 4
    everything = struct.pack("<4d", -np.inf, np.inf, -np.inf, np.inf) * 32
    # sideways: other rectangles; below the plane every box lies beyond it as seen from the light, on its height the
    # projection is undefined: no rectangle at all, either way
    assert f[0]["rects"] != f[1]["rects"] and everything not in (f[0]["rects"], f[1]["rects"])
    assert f[2]["rects"] == f[3]["rects"] == everything
    assert f[0] == f[4]


def test_light2_of_three_leaves_the_rectangles(tmp_path):
    f = _run("light2_of_three", tmp_path)
    assert f[0]["rects"] == f[1]["rects"] and f[0]["lights"] != f[1]["lights"] and f[0]["lpos"] != f[1]["lpos"]
    assert f[1]["rects"] != f[2]["rects"]


def test_light_power_and_colour(tmp_path):
    f = _run("light_values", tmp_path)
    lit = [struct.unpack_from("<I", s["lights"], 36)[0] for s in f]  # DevLight::lit
    assert lit == [3, 2, 3, 1, 3]  # power 0: not lit; 2^70: outside the lean window of the 1/r^2 numerators
    assert f[0] == f[2] == f[4]


def test_nan_and_infinity_unbox_the_node(tmp_path):
    f = _run("nan_inf", tmp_path)
    assert [s["boxed"][3] for s in f] == [1, 0, 0, 1]
    assert f[0] == f[3]


def test_forty_nodes_both_sides_of_the_mask_width(tmp_path):
    f = _run("forty", tmp_path)
    for a, b in zip(f, f[1:]):
        assert a["nodes"] != b["nodes"]
    assert f[0]["rects"] != f[1]["rects"]   # node 31 has a rectangle
    assert f[1]["rects"] == f[2]["rects"]   # node 32 has none: beyond kMaxCullNodes


def test_descending_order_gives_the_same_plan(tmp_path):
    scene = U.load_case_scene("l5", tmp_path)
    base = U.Desc(scene.desc)
    nodes = {1: U.xf(("translate", 3, 4, 5)), 3: U.xf(("scale", 2, 2, 2)), 5: U.xf(("translate", -9, 15, 100))}
    up, down = Uploaded(base.d), Uploaded(base.d)
    assert up.apply(c2.makePose(nodes, None))[0] == _abi.OK
    assert down.apply(c2.makePose(dict(reversed(list(nodes.items()))), None))[0] == _abi.OK
    assert up.plan() == down.plan() == fresh_plan(base.patched(nodes).d)


def test_refusals_leave_the_plan_as_it_was(tmp_path):
    scene = U.load_case_scene("l5x3", tmp_path)
    base = U.Desc(scene.desc)
    up = Uploaded(base.d)
    assert up.apply(c2.makePose({1: U.xf(("translate", 1, 2, 3))}, {1: dict(power=5.0)}))[0] == _abi.OK  # state to keep
    before = up.plan()
    t = U.xf(("translate", 9, 9, 9))

    def raw(**kw):
        pose = _abi.ScenePose()
        keep = []
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data_as(type(getattr(pose, k)))
            setattr(pose, k, v)
        pose._keep = keep
        return pose

    idx = lambda *v: np.array(v, dtype=np.uint32)
    pos = np.zeros(6, dtype=np.float64)
    two = np.concatenate([t, t])
    cases = [
        (None, "null pose"),
        (raw(n_nodes=1, node_transform=t), "pose: 1 nodes with a null node_index"),
        (raw(n_lights=2, light_pos=pos), "pose: 2 lights with a null light_index"),
        (raw(n_nodes=1, node_index=idx(0)), "pose: 1 nodes with a null node_transform"),
        (raw(n_lights=1, light_index=idx(0)), "pose: 1 lights with null light_pos, light_color and light_power"),
        (raw(n_nodes=2, node_index=idx(2, 6), node_transform=two), "pose: node_index[1] = 6 out of range (the scene has 6 nodes)"),
        (raw(n_lights=1, light_index=idx(3), light_pos=pos), "pose: light_index[0] = 3 out of range (the scene has 3 lights)"),
        (raw(n_nodes=2, node_index=idx(4, 4), node_transform=two), "pose: node_index[1] = 4 is listed twice"),
        (raw(n_lights=2, light_index=idx(1, 1), light_pos=pos), "pose: light_index[1] = 1 is listed twice"),
        # a good node half does not get in when the light half is refused
        (raw(n_nodes=1, node_index=idx(2), node_transform=t, n_lights=1, light_index=idx(7), light_pos=pos),
         "pose: light_index[0] = 7 out of range (the scene has 3 lights)"),
    ]
    for pose, want in cases:
        st, msg = up.apply(pose)
        assert (st, msg) == (_abi.ERR_INVALID_ARG, want)
        assert up.plan() == before, want
    # an empty pose is fine and changes nothing
    assert up.apply(_abi.ScenePose())[0] == _abi.OK and up.plan() == before


def test_lecture5_itself_keeps_its_texels(scenes_dir):
    """lecture5.sdl with its two bitmaps: the replanned plan carries the float4 pool it had (6 MB, byte for byte the
    fresh plan's), without the description's texels being there to convert again."""
    import chess2rt_amd

    scene = chess2rt_amd.parseSceneFromFile(os.path.join(scenes_dir, "lecture5.sdl"))
    base = U.Desc(scene.desc)
    up = Uploaded(base.d)
    base.a["texels"][:] = -1.0  # the caller's pool is gone after the upload: an update must not read it
    nodes = {3: U.xf(("translate", 60, 15, 200)), 4: U.xf(("scale", 1, 2, 1), ("translate", 0, 30, 150))}
    assert up.apply(c2.makePose(nodes, {0: dict(pos=(0, 500, 100))}))[0] == _abi.OK
    want = U.Desc(scene.desc).patched(nodes, {0: dict(pos=(0, 500, 100))})
    assert_same_plan(up.plan(), fresh_plan(want.d), "lecture5")
    assert len(sections(up.plan())["texels4"]) > (1 << 20)

"""Path planes, CPU side: the ABI (a C program against the headers, the five entry points refusing a null context), the
Python layer's argument checks, the family object against its struct, the walk of tests/paths_reference.py on hand-made
inputs, and the precondition of the GPU tests, asserted on the oracle alone.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import occlusion_cases as oc
import paths_reference as pr
from chess2rt_amd import _abi, api
from ray_query_util import oracle_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, B = 8, 4

C_PROGRAM = r"""
#include <stddef.h>
#include <stdint.h>
#include "c2rt.h"
#include "c2rt_host.h"
_Static_assert(sizeof(c2rt_path_opts) == 16, "c2rt_path_opts");
_Static_assert(offsetof(c2rt_path_opts, seed) == 0 && offsetof(c2rt_path_opts, paths) == 8 &&
               offsetof(c2rt_path_opts, bounces) == 12, "c2rt_path_opts members");
_Static_assert(sizeof(c2rt_path_planes) == 40, "c2rt_path_planes");
_Static_assert(offsetof(c2rt_path_planes, node) == 0 && offsetof(c2rt_path_planes, segments) == 8 &&
               offsetof(c2rt_path_planes, indirect) == 16 && offsetof(c2rt_path_planes, bounce) == 24 &&
               offsetof(c2rt_path_planes, radiance) == 32, "c2rt_path_planes members");
_Static_assert(C2RT_MAX_PATHS == 64 && C2RT_MAX_PATH_BOUNCES == 8, "the limits");
_Static_assert(C2RT_ABI_VERSION == 1, "the path planes are additive");
/* the prototypes, as the issue states them */
static int (*const p_frame_dev)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_path_opts *,
                                const c2rt_path_planes *, void *) = c2rt_render_paths_device;
static int (*const p_frame)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_path_opts *,
                            const c2rt_path_planes *) = c2rt_render_paths;
static int (*const p_rays_dev)(c2rt_ctx *, const c2rt_ray *, uint64_t, const c2rt_path_opts *, const c2rt_path_planes *,
                               void *) = c2rt_trace_rays_paths_device;
static int (*const p_rays)(c2rt_ctx *, const c2rt_ray *, uint64_t, const c2rt_path_opts *, const c2rt_path_planes *) = c2rt_trace_rays_paths;
static int (*const p_host)(c2rt_ctx *, c2rt_host_scene *, const c2rt_path_opts *, const c2rt_path_planes *) = c2rt_host_render_paths;
/* the members' types */
static uint64_t *seed_of(c2rt_path_opts *o) { return &o->seed; }
static uint32_t *paths_of(c2rt_path_opts *o) { return &o->paths; }
static uint32_t *bounces_of(c2rt_path_opts *o) { return &o->bounces; }
static int32_t *node_of(c2rt_path_planes *p) { return p->node; }
static uint32_t *segments_of(c2rt_path_planes *p) { return p->segments; }
static float *indirect_of(c2rt_path_planes *p) { return p->indirect; }
static float *bounce_of(c2rt_path_planes *p) { return p->bounce; }
static float *radiance_of(c2rt_path_planes *p) { return p->radiance; }
int opts_size(void)
{
    c2rt_path_opts o = {0};
    return (int)sizeof o + (*seed_of(&o) || *paths_of(&o) || *bounces_of(&o));
}
int planes_size(void)
{
    c2rt_path_planes pl = {0};
    return (int)sizeof pl + (node_of(&pl) || segments_of(&pl) || indirect_of(&pl) || bounce_of(&pl) || radiance_of(&pl));
}
void null_context(int *st)
{
    c2rt_ray ray = {{0, 0, 0}, {0, 0, 1}};
    int32_t node;
    c2rt_camera_frame cam = {{0}};
    c2rt_render_opts opts = {0};
    c2rt_path_opts g = {0, 1, 1};
    c2rt_path_planes planes = {0};
    planes.node = &node;
    st[0] = p_frame_dev(NULL, &cam, &opts, &g, &planes, NULL);
    st[1] = p_frame(NULL, &cam, &opts, &g, &planes);
    st[2] = p_rays_dev(NULL, &ray, 1, &g, &planes, NULL);
    st[3] = p_rays(NULL, &ray, 1, &g, &planes);
    st[4] = p_host(NULL, NULL, &g, &planes);
}
"""


def test_header_layout_and_null_context(tmp_path):
    src = tmp_path / "paths.c"
    src.write_text(C_PROGRAM)
    so = tmp_path / "libpaths_probe.so"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)])
    lib = _abi.load_library()                # RTLD_GLOBAL: the probe's undefined symbols resolve to libc2rt.so's
    probe = C.CDLL(str(so))
    assert probe.opts_size() == 16 == C.sizeof(_abi.PathOpts)
    assert probe.planes_size() == 40 == C.sizeof(_abi.PathPlanes)
    assert [(f[0], getattr(_abi.PathOpts, f[0]).offset) for f in _abi.PathOpts._fields_] == [("seed", 0), ("paths", 8), ("bounces", 12)]
    assert [f[0] for f in _abi.PathPlanes._fields_] == ["node", "segments", "indirect", "bounce", "radiance"]
    st = (C.c_int * 5)(*([-1] * 5))
    probe.null_context(st)
    assert list(st) == [_abi.ERR_INVALID_ARG] * 5
    for name in ("c2rt_render_paths_device", "c2rt_render_paths", "c2rt_trace_rays_paths_device", "c2rt_trace_rays_paths"):
        assert name in _abi.C2RT_SYMBOLS and hasattr(lib, name)
    assert "c2rt_host_render_paths" in _abi.C2RT_HOST_SYMBOLS and hasattr(lib, "c2rt_host_render_paths")
    assert _abi.ABI_VERSION == 1 == lib.c2rt_abi_version()


def test_python_layer_checks_its_arguments_before_the_library():
    """an unknown plane name and a wrong ray shape are refused by the Python layer: no context is touched"""
    with pytest.raises(ValueError):
        api._PATHS.new(("node", "hits"), (4,))
    with pytest.raises(ValueError):
        api._PATHS.device({"open": 1})
    pl, out = api._PATHS.new(("segments", "radiance"), (3, 5))
    assert list(out) == ["segments", "radiance"] and out["segments"].shape == (3, 5) and out["radiance"].shape == (3, 5, 3)
    assert out["segments"].dtype == np.uint32 and out["radiance"].dtype == np.float32
    assert pl.node is None and pl.indirect is None and pl.bounce is None
    assert pl.segments == out["segments"].ctypes.data and pl.radiance == out["radiance"].ctypes.data
    dev = api._PATHS.device({"node": 64, "indirect": 0})
    assert dev.node == 64 and all(getattr(dev, n) is None for n in ("segments", "indirect", "bounce", "radiance"))
    g = api._path_opts(16, 4, (1 << 40) + 5)
    assert (g.paths, g.bounces, g.seed) == (16, 4, (1 << 40) + 5)

    class NoContext:
        _lib = _h = None
    with pytest.raises(ValueError):
        api.Context.traceRaysPaths(NoContext(), np.zeros((4, 5)), 8, 4)
    import chess2rt_amd as c2
    for name in ("PathOpts", "PathPlanes", "PATH_PLANES"):
        assert name in c2.__all__ and hasattr(c2, name)
    for name in ("renderPaths", "renderPathsDevice", "traceRaysPaths", "traceRaysPathsDevice"):
        assert callable(getattr(api.Context, name))
    assert callable(api.Renderer.renderPaths)


# ---- the family object against its struct: the checks of tests/test_plane_families.py, for _PATHS ------------------------

FAM, TABLE, STRUCT, SAMPLE_BYTES, NOUN = api._PATHS, api.PATH_PLANES, _abi.PathPlanes, 44, "path"


def test_table_is_the_struct():
    assert FAM.table is TABLE and FAM.struct is STRUCT
    assert list(TABLE) == [f[0] for f in STRUCT._fields_]
    assert C.sizeof(STRUCT) == len(TABLE) * C.sizeof(C.c_void_p)      # nothing but pointers
    assert sum(np.dtype(d).itemsize * c for d, c in TABLE.values()) == SAMPLE_BYTES
    assert [np.dtype(d).itemsize * c for d, c in TABLE.values()] == [4, 4, 12, 12, 12]


@pytest.mark.parametrize("shape", [(5,), (3, 4)])
def test_new_allocates_the_planes_named_and_no_other(shape):
    names = list(TABLE)
    for asked in (names, names[1::2], names[:1], []):
        pl, out = FAM.new(iter(asked), shape)
        assert isinstance(pl, STRUCT) and list(out) == asked
        for n in names:
            if n not in asked:
                assert getattr(pl, n) is None, n
                continue
            dtype, comps = TABLE[n]
            assert out[n].dtype == np.dtype(dtype) and out[n].flags["C_CONTIGUOUS"], n
            assert out[n].shape == (shape if comps == 1 else shape + (comps,)), n
            assert getattr(pl, n) == out[n].ctypes.data, n


def test_device_keeps_pointers_and_maps_zero_and_none_to_null():
    names = list(TABLE)
    ptrs = {n: 256 * (k + 1) for k, n in enumerate(names)}
    pl = FAM.device(ptrs)
    assert isinstance(pl, STRUCT) and [getattr(pl, n) for n in names] == list(ptrs.values())
    pl = FAM.device({names[0]: 0, names[1]: None, names[-1]: 4096})
    assert getattr(pl, names[0]) is None and getattr(pl, names[1]) is None and getattr(pl, names[-1]) == 4096
    assert all(getattr(pl, n) is None for n in names[2:-1])
    assert all(getattr(FAM.device({}), n) is None for n in names)


def test_unknown_name_is_refused_in_the_words_of_the_family():
    want = "unknown path plane 'depth_of' (one of node, segments, indirect, bounce, radiance)"
    with pytest.raises(ValueError) as e:
        FAM.new(("node", "depth_of"), (2, 2))
    assert str(e.value) == want
    with pytest.raises(ValueError) as e:
        FAM.device({"depth_of": 64})
    assert str(e.value) == want


# ---- the walk on hand-made inputs ------------------------------------------------------------------------------------------


def hand_made():
    """three samples: a hit on a floor facing +y, a miss, a hit seen from below (the normal is turned)"""
    rec = np.zeros(3, dtype=api.RAY_HIT_DTYPE)
    rec["closest_node"] = [2, -1, 0]
    rec["normal"] = [[0, 1, 0], [0, 0, 0], [0, -1, 0]]
    rec["p"] = [[1, 0, 2], [0, 0, 0], [3, 0, 4]]
    dirs = np.array([[0, -1, 0], [0, 0, 1], [0, -1, 0.0]])
    return rec, dirs


def test_reference_walk_of_hand_made_inputs():
    rec, dirs = hand_made()
    f = np.float32
    P2, B2, seed = 2, 3, 1
    w = pr.Walk(rec, dirs, np.arange(3), P2, B2, seed)
    assert w.hit.tolist() == [True, False, True]
    s, p = w.alive()
    assert s.tolist() == [0, 0, 2, 2] and p.tolist() == [0, 1, 0, 1]            # a miss draws nothing
    r0 = w.rays(0)
    assert np.array_equal(r0[:2, :3], [[1, 1e-6, 2]] * 2) and np.array_equal(r0[2:, :3], [[3, 1e-6, 4]] * 2)
    assert (r0[:, 4] >= 0).all()                                               # flipped into the hemisphere of +y
    # depth 0 draws the gather planes' directions: key (seed, idx, 0), sample = path
    import gather_reference as gr
    _, _, sp = gr.spawned(rec, dirs, np.arange(3), P2, seed)
    assert r0.tobytes() == np.ascontiguousarray(sp[[0, 0, 2, 2], [0, 1, 0, 1]]).tobytes()
    w0 = pr.weight(r0[:, 3:], np.array([[0, 1, 0.0]] * 4))
    assert w0.dtype == f and np.array_equal(w0, (2.0 * r0[:, 4]).astype(f))
    # depth 0: sample 0's path 0 hits a wall facing -x, its path 1 misses; sample 2's paths both hit the wall
    L0 = np.array([[0.5, 0.25, 1.0], [0, 0, 0], [0.125, 2.0, 0.75], [1.0, 1.0, 1.0]], dtype=f)
    a1 = np.array([[0.5, 0.5, 0.25], [9, 9, 9], [0.75, 0.5, 1.0], [0.3, 0.6, 0.9]], dtype=f)
    wall_n = np.array([[1.0, 0, 0]] * 4)
    wall_p = np.array([[5.0, 1, 2], [0, 0, 0], [5.0, 2, 4], [5.0, 3, 4]])
    w.answers(0, [7, -1, 7, 7], L0, a1, wall_n, wall_p)
    s, p = w.alive()
    assert s.tolist() == [0, 2, 2] and p.tolist() == [0, 0, 1]                   # the path that missed is over
    r1 = w.rays(1)
    N1 = pr.ocr.faceforward(r0[[0, 2, 3], 3:], wall_n[:3])
    assert np.array_equal(r1[:, :3], wall_p[[0, 2, 3]] + N1 * 1e-6)
    # depth 1 draws under key (seed, idx, 1)
    assert r1[:, 3:].tobytes() == pr.directions(seed, [0, 2, 2], 1, [0, 0, 1], N1).tobytes()
    assert r1[:, 3:].tobytes() != pr.directions(seed, [0, 2, 2], 0, [0, 0, 1], N1).tobytes()
    w1 = pr.weight(r1[:, 3:], N1)
    L1 = np.array([[0.2, 0.4, 0.6], [0, 0, 0], [0.7, 0.1, 0.3]], dtype=f)
    a2 = np.array([[0.9, 0.8, 0.7], [9, 9, 9], [0.6, 0.5, 0.4]], dtype=f)
    w.answers(1, [3, -1, 3], L1, a2, wall_n[:3], wall_p[[0, 2, 3]] + 1.0)
    r2 = w.rays(2)
    assert len(r2) == 2
    N2 = w.N[[0, 2], [0, 1]]
    w2 = pr.weight(r2[:, 3:], N2)
    L2 = np.array([[1.5, 0.5, 0.25], [0.4, 0.8, 1.2]], dtype=f)
    w.answers(2, [1, 1], L2, a2[:2], wall_n[:2], wall_p[:2])
    a0 = np.array([[0.5, 0.25, 2.0], [1, 1, 1], [0.1, 0.2, 0.3]], dtype=f)
    rgb0 = np.array([[0.25, 0.5, 0.75], [0, 0, 0], [1, 2, 3]], dtype=f)
    pl = w.planes(a0, rgb0)
    assert pl["node"].tolist() == [2, -1, 0] and pl["segments"].tolist() == [3, 0, 4]
    assert w.hits_at == [3, 2, 2]
    # sample 0 by hand: path 0 has three segments, path 1 one (a miss: + 0 * w, executed)
    T0 = f(w0[0])
    T1 = (T0 * a1[0]).astype(f) * w1[0]
    T2 = (T1 * a2[0]).astype(f) * w2[0]
    want = f(0) + L0[0] * T0
    want = want + L1[0] * T1
    want = want + L2[0] * T2
    want = want + L0[1] * f(w0[1])
    assert pl["indirect"][0].tobytes() == (want / f(P2)).astype(f).tobytes()
    assert pl["bounce"][0].tobytes() == (a0[0] * pl["indirect"][0]).tobytes()
    assert pl["radiance"][0].tobytes() == (rgb0[0] + pl["bounce"][0]).tobytes()
    # the miss: +0 everywhere, radiance the ray's colour
    for name in ("indirect", "bounce"):
        assert not pl[name][1].view(np.uint32).any()
    assert pl["radiance"][1].tobytes() == rgb0[1].tobytes()
    # Beff == 0 draws nothing
    z = pr.Walk(rec, dirs, np.arange(3), P2, 0, seed)
    assert len(z.rays(0)) == 0
    zp = z.planes(a0, rgb0)
    assert zp["node"].tolist() == [2, -1, 0] and not zp["segments"].any()
    assert not zp["indirect"].view(np.uint32).any() and not zp["bounce"].view(np.uint32).any()
    assert zp["radiance"].tobytes() == rgb0.tobytes()


def test_the_order_of_the_sum_is_part_of_the_contract():
    """path-major, bounce-minor: with terms 1e8, 1, -1e8, 1 over two paths of two segments, the other nest gives
    another float"""
    rec, dirs = hand_made()
    rec, dirs = rec[:1], dirs[:1]
    f = np.float32
    w = pr.Walk(rec, dirs, [0], 2, 2, 3)
    r0 = w.rays(0)
    up = np.array([[0, 1, 0.0]] * 2)
    w0 = pr.weight(r0[:, 3:], up)
    # colours chosen so that L * T is exactly the wanted term where w is a power of two away; take the terms as they
    # come and compare the two orders on whatever they are
    w.answers(0, [1, 1], (np.array([[1e8] * 3, [-1e8] * 3]) / w0[:, None]).astype(f), np.ones((2, 3), dtype=f), up, [[0, 0, 0], [1, 0, 1]])
    r1 = w.rays(1)
    w1 = pr.weight(r1[:, 3:], w.N[[0, 0], [0, 1]])
    w.answers(1, [-1, -1], (np.ones((2, 3)) / (w0 * w1)[:, None]).astype(f), np.ones((2, 3), dtype=f), up, [[0, 0, 0]] * 2)
    t = w.term[0]                                        # (path, depth, 3)
    assert abs(t[0, 0, 0]) > 1e7 and abs(t[1, 0, 0]) > 1e7 and 0.5 < t[0, 1, 0] < 2 and 0.5 < t[1, 1, 0] < 2
    ours = w.planes(np.ones((1, 3), dtype=f), np.zeros((1, 3), dtype=f))["indirect"][0]
    other = w.planes(np.ones((1, 3), dtype=f), np.zeros((1, 3), dtype=f), order="bounce-major")["indirect"][0]
    by_hand = (((f(0) + t[0, 0]) + t[0, 1]) + t[1, 0]) + t[1, 1]
    assert ours.tobytes() == (by_hand / f(2)).astype(f).tobytes()
    assert ours.tobytes() != other.tobytes()


# ---- the precondition of the GPU tests, on the oracle alone -----------------------------------------------------------------


def oracle_ask(desc):
    def ask(rays):
        r = oracle_trace(desc, rays)
        zeros = np.zeros((len(rays), 3), dtype=np.float32)
        return r["closest_node"], zeros, zeros, r["normal"], r["p"]
    return ask


@pytest.mark.parametrize("which", oc.RAY_SETS)
@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_every_vertex_has_hitting_segments(name, which):
    """the inputs are worth testing: following the oracle through the definition at seed 7 with 8 paths and 4 bounces,
    at least 100 segments hit a node at every vertex 1 .. 4"""
    scene, _, _ = oc.load(name)
    rays = oc.ray_set(name, which)
    recs = oracle_trace(scene.desc, rays)
    w, asked = pr.walk(recs, rays[:, 3:], np.arange(len(rays)), P, B, oc.SEED, oracle_ask(scene.desc))
    print("%s %s, P = %d, B = %d, seed %d: %d hits, segments asked per depth %s, hitting %s"
          % (name, which, P, B, oc.SEED, int(w.hit.sum()), [len(a) for a in asked], w.hits_at))
    assert len(w.hits_at) == B and min(w.hits_at) >= 100
    assert int(w.segments.sum()) == sum(w.hits_at) and (w.segments <= P * B).all() and not w.segments[~w.hit].any()

"""The planner's kCsgCertain flag (scene_plan.cpp: csg_certain_ok; c2rt_device.h): on for lecture5's CsgDiff(Cube, Sphere),
off for a Plane child, Op(a, a), a non-finite cube, a nested child and geometry beyond the domain csg_certain.h's bounds
were derived for; drop_csg_certain (C2RT_DEBUG_CULL bit 9 of the diagnostics build) clears it everywhere.  Through
tests/csg_certain_check.cpp, which runs plan_scene itself."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import chess2rt_amd as c2  # noqa: E402
from chess2rt_amd import _abi  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl")
K_CSG_CERTAIN = 16


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "tests", "libcsg_certain_check.so")
    if not os.path.exists(path):
        pytest.fail("tests/libcsg_certain_check.so is missing: run `make all` (build())")
    return C.CDLL(path)


def flags_of(lib, mutate=None, drop=0):
    s = c2.parseSceneFromFile(SCENE)
    d = s.desc.contents
    g = next(d.node_geom[n] for n in range(d.n_nodes) if d.geom_type[d.node_geom[n]] >= _abi.GEOM_CSG_UNION)
    l, r = d.geom_child[2 * g], d.geom_child[2 * g + 1]
    if mutate:
        mutate(d, g, l, r)
    out = np.zeros(d.n_geoms, dtype=np.int32)
    st = lib.csg_certain_plan_flags(s.desc, drop, out.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint32(d.n_geoms))
    assert st == 0, st
    return int(out[g]), out


def test_lecture5_tree_is_eligible(lib):
    f, every = flags_of(lib)
    assert f & K_CSG_CERTAIN
    assert int(((every & K_CSG_CERTAIN) != 0).sum()) == 1       # the CsgOp alone: primitives never carry it
    f, every = flags_of(lib, drop=1)
    assert not (every & K_CSG_CERTAIN).any()


def _param(c, i, v):
    def m(d, g, l, r):
        d.geom_param[4 * (l if c == "l" else r) + i] = v
    return m


def _plane_child(d, g, l, r):
    d.geom_type[r] = _abi.GEOM_PLANE


def _same_child(d, g, l, r):
    d.geom_child[2 * g + 1] = l


def _nested_child(d, g, l, r):
    # the right child becomes a CsgOp of its own over two primitives that are not in the tree yet
    others = [k for k in range(d.n_geoms) if k not in (g, l, r) and d.geom_type[k] in (_abi.GEOM_SPHERE, _abi.GEOM_CUBE)]
    assert len(others) >= 2
    d.geom_type[r] = _abi.GEOM_CSG_UNION
    d.geom_child[2 * r], d.geom_child[2 * r + 1] = others[0], others[1]


OFF = {
    "plane_child": _plane_child,
    "op_a_a": _same_child,
    "cube_side_inf": _param("l", 3, float("inf")),
    "cube_centre_nan": _param("l", 0, float("nan")),
    "nested_child": _nested_child,
    "centre_beyond_2^20": _param("l", 2, 2.0 ** 21),
    "side_beyond_2^20": _param("l", 3, 2.0 ** 21),
    "radius_below_2^-10": _param("r", 3, 2.0 ** -11),
    "radius_negative": _param("r", 3, -70.0),
}


@pytest.mark.parametrize("name", sorted(OFF))
def test_ineligible_trees(lib, name):
    f, _ = flags_of(lib, OFF[name])
    assert not (f & K_CSG_CERTAIN), name


@pytest.mark.parametrize("name,mutate", [("centre_at_2^20", _param("l", 2, 2.0 ** 20)), ("radius_at_2^-10", _param("r", 3, 2.0 ** -10))])
def test_domain_edges_are_inside(lib, name, mutate):
    f, _ = flags_of(lib, mutate)
    assert f & K_CSG_CERTAIN, name

"""Which nodes, and which tiles, the planner hands to lean::csg_tile (chess2rt_amd/csrc/c2rt_trace.inc): the kNodeCsgTile
flags of scene_plan.cpp's plan_csg_tile_nodes in a frame with RenderParams::ground_fast, through the host build
tests/libcsg_tile_check.so, and render_tile's condition on the planner's own mask words (scripts/csg_tile_census.py) —
no GPU."""
import os
import sys

import numpy as np
import pytest

import chess2rt_amd as c2
from chess2rt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import csg_tile_census as census  # noqa: E402
import csg_tile_scenes as S  # noqa: E402
import csg_void_tiles as cv  # noqa: E402


def _load(tmp_path, name, edit=None, size=(64, 48), **case):
    path = tmp_path / (name + ".sdl")
    path.write_text(S.text(edit))
    for f in ("floor.bmp", "world.bmp"):
        if not (tmp_path / f).exists():
            (tmp_path / f).write_bytes(open(os.path.join(S.SCENES, f), "rb").read())
    scene = c2.parseSceneFromFile(str(path))
    scene.setFrameSize(*size)
    S.rewrite(scene, case)
    return scene, scene.beginFrame(), scene.renderOpts(taps=5)


@pytest.mark.parametrize("size,tiles,claimed", [((3840, 2160), 129600, 14081), ((1920, 1080), 32400, 4378)])
def test_lecture5_as_shipped(tmp_path, size, tiles, claimed):
    """node 2 (the CsgDiff), and the tile counts of the host histogram of the first two mask words"""
    scene, cam, opts = _load(tmp_path, "lecture5", size=size)
    eligible, ground, plan_mask = census.eligible_nodes(scene.desc, cam, opts)
    assert (eligible, ground, plan_mask) == (1 << 2, 0, 1 << 2)
    W, H = size
    bounds = [cv.tile_bounds(r, c, 0, H) for r in range((H + 7) // 8) for c in range((W + 7) // 8)]
    node, pm, sm = census.claimed_tiles(scene.desc, cam, opts, bounds)
    assert node.size == tiles and int((node == 2).sum()) == claimed and int((node >= 0).sum()) == claimed
    # every tile that keeps the CsgDiff node in its primary mask keeps exactly {ground, CsgDiff} in both masks
    keeps = (pm & np.uint32(4)) != 0
    assert np.array_equal(keeps, node == 2)
    # the diagnostics switch
    assert census.eligible_nodes(scene.desc, cam, opts, census.NO_PATH) == (0, 0, 0)
    assert int((census.claimed_tiles(scene.desc, cam, opts, bounds[:4000], census.NO_PATH)[0] >= 0).sum()) == 0


@pytest.mark.parametrize("edit,case", [
    (None, dict(op=3)), (None, dict(op=4, pair="sc")), (None, dict(pair="ss")), (None, dict(op=3, pair="cc_shared_face")),
    ("lambert", {}), ("checker", {}), ("plain", {}), ("light_below", {}), ("power_0", {}), ("csg_first", {}),
    (None, dict(translate=[30.0, 5.0, -20.0])),
], ids=lambda v: "_".join("%s" % x for x in v.values()) if isinstance(v, dict) else str(v))
def test_eligible_scenes(tmp_path, edit, case):
    scene, cam, opts = _load(tmp_path, "s", edit, **case)
    node, _ = S.csg_node(scene.desc.contents)
    eligible, ground, plan_mask = census.eligible_nodes(scene.desc, cam, opts)
    assert eligible == plan_mask == 1 << node and ground == (1 if edit == "csg_first" else 0)


@pytest.mark.parametrize("edit,case", [
    (None, dict(inel="nested")), (None, dict(inel="plane")), (None, dict(rotate=[25.0, 10.0, 5.0])), ("csg_textured", {}), ("two_lights", {}),
], ids=["nested_csgop", "plane_child", "non_identity_matrix", "textured_node", "two_lights"])
def test_refused_scenes(tmp_path, edit, case):
    scene, cam, opts = _load(tmp_path, "s", edit, **case)
    eligible, _, plan_mask = census.eligible_nodes(scene.desc, cam, opts)
    assert eligible == 0 and plan_mask == 0


def test_refused_frames(tmp_path):
    """depth of field, stereo, a counted frame, no light at all: the plan keeps its flag, the frame grants nothing (no ground_fast)"""
    scene, cam, opts = _load(tmp_path, "s")
    assert census.eligible_nodes(scene.desc, cam, opts)[0] == 4
    dof = _abi.CameraFrame.from_buffer_copy(cam)
    dof.dof, dof.num_samples = 1, 4
    stereo = _abi.CameraFrame.from_buffer_copy(cam)
    stereo.stereo_separation = 2.0
    # (a scene without a light has no ground node in the planner's sense, hence no ground_fast frame: its one light
    # switched off — power 0 — is the eligible way to render unlit)
    dark, dcam, dopts = _load(tmp_path, "dark", no_light=True)
    assert census.eligible_nodes(dark.desc, dcam, dopts) == (0, -1, 4)
    for c, o in ((dof, opts), (stereo, opts), (cam, scene.renderOpts(taps=5, count_rays=1))):
        eligible, _, plan_mask = census.eligible_nodes(scene.desc, c, o)
        assert eligible == 0 and plan_mask == 4
        assert int((census.claimed_tiles(scene.desc, c, o, [cv.tile_bounds(r, k, 0, 48) for r in range(6) for k in range(8)])[0] >= 0).sum()) == 0

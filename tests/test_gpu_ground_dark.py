"""Dark ground tiles on the device (chess2rt_amd/csrc/csg_void.h: tile_dark_by; c2rt_tile_mask.inc: tile_mask_entry writes
bit 2 of the mask table's third word, lean::ground_tile renders such a tile without shadow rays and light terms).

lecture5 at 640x480 — the smallest size with enough dark tiles to show anything — as a whole frame, as two ranks' 8-row
strips and as a batch of two cameras through c2rt_render_frames_device, each rendered in a child process on the
diagnostics library, once as shipped and once with C2RT_DEBUG_CULL=32 (no dark test).  In each case the device's dark
bits (c2rt_debug_tile_masks, tests/csg_void_device.py) equal the host classifier's claims tile for tile
(scripts/ground_dark_tiles.py, which tests/test_ground_dark_tiles.py checks ray by ray in the oracle), the two frames
are the same bits, the frame equals the oracle's float for float, and c2rt_get_exact_redos does not move."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

_CHILD = r'''
import json, os, sys
sys.path[:0] = [os.path.join(os.getcwd(), "tests"), os.path.join(os.getcwd(), "scripts")]
import numpy as np
import chess2rt_amd as c2, csg_void_device as vdev, csg_void_tiles as cv, ground_dark_tiles as gd, oracle_lib as orc
outdir, with_oracle = sys.argv[1], sys.argv[2] == "1"
debug_cull = int(os.environ.get("C2RT_DEBUG_CULL", "0"))
W, H = 640, 480
ctx = c2.Context(0)
scene = c2.parseSceneFromFile(os.path.join("tests", "golden", "scenes", "lecture5.sdl"))
scene.setFrameSize(W, H)
cam0 = scene.beginFrame()
scene.rotateCamera(20, 0, 5)
scene.moveCamera(-30, 10, 40)
cam1 = scene.beginFrame()
ctx.uploadScene(scene.desc)

def dark_bits(cam, opts):
    """(device dark bits, host claims under the device's primary-ground bit, primary-ground bits) of the frame's table"""
    m, info, _ = vdev.read_tile_masks(ctx, cam, opts, 3)
    bounds = [cv.tile_bounds(r, c, info["mask_row0"], info["mask_rows"], opts.strip_height or 1,
                             opts.strip_rank if opts.strip_world > 1 else 0, max(opts.strip_world, 1))
              for r in range(info["tile_rows"]) for c in range(info["cols"])]
    frame = gd.dark_frame(scene.desc, cam, opts, debug_cull)
    host = np.zeros((info["tile_rows"], info["cols"]), dtype=bool)
    for j in range(frame.d.n):
        host |= gd.classify_tiles(cam, bounds, frame.d.d[j], frame).reshape(host.shape) != 0
    w2 = m[..., 2]
    assert not np.any(m[..., 3])
    return (w2 & 4) != 0, host & ((w2 & 1) != 0), (w2 & 1) != 0, (w2 & 2) != 0

for name, cams, ranks, sh in (("whole", [cam0], 1, 0), ("strips", [cam0], 2, 8), ("batch", [cam0, cam1], 1, 0)):
    arrays, dark, differ, outside = {}, 0, 0, 0
    redos0 = ctx.exactRedos()
    for rank in range(ranks):
        kw = dict(taps=5)
        if ranks > 1:
            kw.update(strip_height=sh, strip_rank=rank, strip_world=ranks)
        opts = scene.renderOpts(**kw)
        for cam in cams:
            dev, host, pg, go = dark_bits(cam, opts)
            dark += int(dev.sum())
            differ += int((dev != host).sum())
            outside += int((dev & (~pg | go)).sum())  # dark only among primary-ground tiles that are not ground-only
        if name == "batch":
            import torch
            buf = torch.zeros((len(cams), ctx.localRows(opts), opts.width, 3), dtype=torch.float32, device="cuda")
            ctx.renderFramesDevice(cams, opts, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = list(buf.cpu().numpy())
        else:
            got = [ctx.renderFrame(cams[0], opts)]
        for i, f in enumerate(got):
            arrays["frame_%d_%d" % (rank, i)] = f
            if with_oracle:
                arrays["ref_%d_%d" % (rank, i)] = orc.render_frame(scene.desc, cams[i], opts, 0)
    np.savez(os.path.join(outdir, name + ".npz"), **arrays)
    print(json.dumps(dict(name=name, dark=dark, differ=differ, outside=outside, redos=int(ctx.exactRedos() - redos0),
                          frames=sorted(k for k in arrays if k.startswith("frame")))), flush=True)
print("ok")
'''

CASES = ("whole", "strips", "batch")


def _run_child(outdir, env_extra, with_oracle):
    os.makedirs(outdir)
    env = dict(os.environ, C2RT_LIB_VARIANT="diag", **env_extra)
    p = subprocess.run([sys.executable, "-c", _CHILD, outdir, "1" if with_oracle else "0"], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout[-4000:] + p.stderr[-4000:]
    return {r["name"]: r for r in (json.loads(line) for line in p.stdout.splitlines() if line.startswith("{"))}, p.stderr


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """the three cases as shipped (with the oracle's frames), then with C2RT_DEBUG_CULL=32: two child processes in all"""
    base = tmp_path_factory.mktemp("ground_dark")
    on, _ = _run_child(str(base / "on"), {}, True)
    off, err = _run_child(str(base / "off"), dict(C2RT_DEBUG_CULL="32"), False)
    assert "C2RT_DEBUG_CULL=32" in err  # the hook announces itself, as for the other bits
    assert set(on) == set(off) == set(CASES)
    return base, on, off


@pytest.mark.parametrize("name", CASES)
def test_dark_tiles_on_the_device(rendered, name):
    base, on, off = rendered
    r_on, r_off = on[name], off[name]
    print("%s: %d dark tiles (switch off: %d), %d differ from the host, redos %d / %d" %
          (name, r_on["dark"], r_off["dark"], r_on["differ"], r_on["redos"], r_off["redos"]))
    # the device's dark bits are the host classifier's, tile for tile; none with the switch off; not vacuous
    assert r_on["differ"] == 0 and r_on["outside"] == 0
    assert r_off["dark"] == 0 and r_off["differ"] == 0
    assert r_on["dark"] >= 30, "vacuous: the frame has no dark tiles for the path to render"
    assert r_on["redos"] == r_off["redos"]
    a, b = np.load(str(base / "on" / (name + ".npz"))), np.load(str(base / "off" / (name + ".npz")))
    assert r_on["frames"] == r_off["frames"] and r_on["frames"]
    for key in r_on["frames"]:
        fa, fb, ref = a[key], b[key], a["ref" + key[len("frame"):]]
        assert fa.shape == fb.shape == ref.shape and np.any(fa)
        nne_off = int((fa.view(np.uint32) != fb.view(np.uint32)).sum())
        nne_ref = int((fa != ref).sum())
        print("  %s: %d values differ from the frame without the path, %d from the oracle's" % (key, nne_off, nne_ref))
        assert nne_off == 0, (name, key, nne_off)
        assert not np.isnan(fa).any() and nne_ref == 0, (name, key, nne_ref)

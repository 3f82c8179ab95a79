"""The short chain's own texel fetch, light quotient and tap average (c2rt_trace.inc: lean::ground_tile_certain;
c2rt_trace_shared.inc: bitmap_filtered_uniform, tap_average; DevLight::equal) at frame level.

Built the way tests/test_gpu_ground_certain.py builds its cases — one child process on the diagnostics library,
lecture5 with lines replaced — and rendered three ways each: the production frame, the COUNTED frame of the same camera
(opts.count_rays: exact:: through the general path) and the CPU oracle's frame.  All three must be the same bits.
Frames are 61x47 (partial edge tiles) and 160x96, at 1 and 5 taps.

Floors: world.bmp (800 x 400: neither square nor a power of two; the scene's second texture, so its first texel is not
texel 0 of the pool), floor.bmp moved behind world.bmp in the scene file (offset 320 000), and 24-bpp bitmaps of 1 x 1,
2 x 3 and 3 x 2 texels written here — under a scaling of 0.01 a bitmap spans 100 world units each way and these frames see
more than a thousand, so samples fall in every texel column and row: tx + 1 == width and ty + 1 == height (both wraps)
and their other sides are all in every frame, in the 1 x 1 bitmap at every sample.
Lights: `1 1 1` (one quotient), `1 0.5 0.25` (three), a channel of 0, power 0, no light, a frame with dark tiles.

Against a vacuous pass: in every case the short chain renders at least 90 % of the frame's ground-only tiles
(c2rt_get_ground_bails against the mask table's count), and the cases that must have ground-only tiles say so."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import test_gpu_ground_certain as GC  # noqa: E402  (the child that renders a case three ways, the case record)
import test_gpu_ground_tiles as G  # noqa: E402  (lecture5 with lines replaced)

pytestmark = pytest.mark.gpu

_TMP = "@TMP@"  # stands for the module's temporary directory in a scene text
_SIZES = [(w, h, t) for w, h in ((61, 47), (160, 96)) for t in (1, 5)]


def _bmp24(width, height, seed):
    """a bottom-up 24-bpp BMP with rows padded to four bytes, every byte of every texel different"""
    row = (3 * width + 3) // 4 * 4
    data = bytearray()
    for y in range(height):
        line = bytearray((seed + 37 * (3 * (y * width + x) + c) * (c + 2)) % 251 + 2 for x in range(width) for c in range(3))
        data += line + bytes(row - len(line))
    header = struct.pack("<2sIHHI", b"BM", 54 + len(data), 0, 0, 54)
    info = struct.pack("<IiiHHIIiiII", 40, width, height, 1, 24, 0, len(data), 2835, 2835, 0, 0)
    return header + info + bytes(data)


_SMALL = {"t1x1.bmp": (1, 1, 5), "t2x3.bmp": (2, 3, 11), "t3x2.bmp": (3, 2, 23)}


def _floor_texture(text, file, scaling):
    old = 'file    "%s"\n      scaling  0.005' % os.path.join(G.SCENES, "floor.bmp")
    assert text.count(old) == 1
    return text.replace(old, 'file    "%s"\n      scaling  %s' % (file, scaling))


def _scenes():
    plain = G._lecture5()
    world_block = plain[plain.index("    // Texutre for the globe:"):plain.index("  Shaders {")]
    floor_block = plain[plain.index("    // Texture for the floor:"):plain.index("    // Texutre for the globe:")]
    assert "world.bmp" in world_block and "floor.bmp" in floor_block and world_block.rstrip().endswith("}")
    s = {}
    # the floor under the globe's bitmap: the scene's second texture, given a scaling of its own
    w = GC._edit(plain, 'name  "world"\n', 'name  "world"\n      scaling  0.005\n')
    s["world_bmp"] = GC._edit(w, 'name    "floor_shader"\n      texture "bmp"', 'name    "floor_shader"\n      texture "world"')
    # the two texture blocks in the other order: floor.bmp behind world.bmp's 320 000 texels
    body = world_block.rstrip()[:-1].rstrip()  # world's block without the closing brace of Textures
    s["floor_bmp_second"] = plain.replace(floor_block + world_block, body + "\n\n" + floor_block.rstrip() + "\n  }\n\n")
    for file in _SMALL:
        s[file[:-4]] = _floor_texture(plain, os.path.join(_TMP, file), "0.01")
    s["light_1_0.5_0.25"] = GC._edit(plain, "color  1 1 1", "color  1 0.5 0.25")
    s["light_channel_0"] = GC._edit(plain, "color  1 1 1", "color  0 1 0.5")
    s["power_0"] = G._lecture5(power="0")
    s["no_light"] = G._lecture5(lights="  Lights {\n  }\n\n")
    return s


# cases without a ground-only tile by construction (tests/test_gpu_ground_tiles.py: a scene without a light has no
# ground node): they hold the route to changing nothing there
_NO_GROUND_TILES = ("no_light",)


def _cases():
    c = []
    for name, sdl in _scenes().items():
        c += [GC._case("%s_%dx%d_t%d" % (name, w, h, t), sdl, w, h, t) for w, h, t in _SIZES]
    plain = G._lecture5()
    c.append(GC._case("dark_tiles", plain, 320, 240))
    c.append(GC._case("dark_tiles_t1_light_1_0.5_0.25", GC._edit(plain, "color  1 1 1", "color  1 0.5 0.25"), 320, 240, 1))
    world = _scenes()["world_bmp"]
    c.append(GC._case("strips_2x8", world, sh=8, world=2))
    c.append(GC._case("rgb32", world, kind="rgb32"))
    c.append(GC._case("batch_two_cameras", world, kind="batch"))
    return c


def test_the_scene_edits_took():
    s = _scenes()
    t = s["floor_bmp_second"]
    textures = t[t.index("  Textures {"):t.index("  Shaders {")]
    assert 0 < textures.index("world.bmp") < textures.index("floor.bmp") and textures.rstrip().endswith("}\n  }")
    assert s["floor_bmp_second"].count("BitmapTexture") == 2 and s["floor_bmp_second"].count("{") == s["floor_bmp_second"].count("}")
    assert len({c["name"] for c in _cases()}) == len(_cases())


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    base = tmp_path_factory.mktemp("ground_texel")
    for file, (w, h, seed) in _SMALL.items():
        (base / file).write_bytes(_bmp24(w, h, seed))
    cases = _cases()
    for c in cases:
        c["sdl"] = c["sdl"].replace(_TMP, str(base))
    with open(str(base / "cases.json"), "w") as f:
        json.dump(cases, f)
    env = dict(os.environ, C2RT_LIB_VARIANT="diag")
    p = subprocess.run([sys.executable, "-c", GC._CHILD, str(base), str(base / "cases.json")], capture_output=True, text=True,
                       timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout[-4000:] + p.stderr[-4000:]
    rows = {r["name"]: r for r in (json.loads(line) for line in p.stdout.splitlines() if line.startswith("{"))}
    assert set(rows) == {c["name"] for c in cases}
    return base, rows


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_the_short_chain_renders_the_general_paths_bits(rendered, case):
    base, rows = rendered
    r, name = rows[case["name"]], case["name"]
    a = np.load(str(base / (name + ".npz")))
    print("%s: %d frames, %d ground-only tiles, %d dark, %d bails, %d redos" % (name, r["n"], r["ground_only"], r["dark"], r["bails"], r["redos"]))
    assert r["n"] >= 1
    for i in range(r["n"]):
        f, counted, ref = a["frame%d" % i], a["counted%d" % i], a["ref%d" % i]
        assert f.shape == counted.shape == ref.shape and not np.isnan(f).any()
        ne_counted = int((f.view(np.uint32) != counted.view(np.uint32)).sum())
        ne_ref = int((f.view(np.uint32) != ref.view(np.uint32)).sum())
        print("  frame %d: %d values differ from the counted frame, %d from the oracle's" % (i, ne_counted, ne_ref))
        assert ne_counted == 0 and ne_ref == 0, (name, i, ne_counted, ne_ref)
    if case["kind"] == "rgb32":
        assert np.array_equal(a["packed"], a["encoded"])
    assert r["redos"] == 0
    # the short chain renders at least 90 % of the ground-only tiles (a bail of a dark tile counts against them too)
    assert r["bails"] <= 0.1 * r["ground_only"], (r["bails"], r["ground_only"], r["dark"])
    if not name.startswith(_NO_GROUND_TILES):
        assert r["ground_only"] >= (8 if case["W"] > 61 else 4), "vacuous: the frame has hardly a ground-only tile"
    if name.startswith("dark_tiles"):
        assert r["dark"] >= 1, "vacuous: no dark tile"

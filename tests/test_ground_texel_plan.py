"""The planner's two decisions behind the short chain's texel fetch and light term (chess2rt_amd/csrc/scene_plan.cpp),
through its host build tests/libground_texel_check.so — no GPU.

bitmap_filtered_uniform (c2rt_trace_shared.inc) addresses the floor's texels with 32-bit byte offsets and a 24-bit row
product: fill_params leaves a frame on ground_tile unless the bitmap ends within the pool's first 2^28 texels and both
sides are below 2^24.  The descriptions here are fabricated (three numbers; nothing is allocated).
DevLight::equal (one light quotient for three channels) is set for bit-equal channels under bit 1 of DevLight::lit,
only; the check library returns lit + 4 * equal."""
import ctypes as C
import os
import struct

import pytest

import chess2rt_amd as c2
from chess2rt_amd import _abi

import test_gpu_ground_tiles as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(os.path.join(ROOT, "tests", "libground_texel_check.so"))
    L.c2rt_ground_texel_cq_of.argtypes = [C.c_void_p, C.POINTER(_abi.CameraFrame), C.POINTER(_abi.RenderOpts), C.c_uint32, C.c_uint32, C.c_uint64]
    L.c2rt_ground_texel_cq_of.restype = C.c_double
    L.c2rt_light_lit_of.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_float]
    L.c2rt_light_lit_of.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def frame(tmp_path_factory):
    path = tmp_path_factory.mktemp("ground_texel_plan") / "lecture5.sdl"
    path.write_text(G._lecture5())
    scene = c2.parseSceneFromFile(str(path))
    scene.setFrameSize(160, 96)
    return scene, scene.beginFrame(), scene.renderOpts(taps=5)


def _cq(lib, frame, width=0, height=0, offset=0):
    scene, cam, opts = frame
    cq = lib.c2rt_ground_texel_cq_of(C.cast(scene.desc, C.c_void_p), C.byref(cam), C.byref(opts), width, height, offset)
    assert cq >= 0, "the scene was refused or its floor has no bitmap"
    return cq


M28, M24 = 1 << 28, 1 << 24

# (width, height, offset, on the route)
_BITMAPS = [
    (256, 256, 0, True),
    (800, 400, 65536, True),
    (1 << 14, 1 << 14, 0, True),              # exactly 2^28 texels from 0
    ((1 << 14) + 1, 1 << 14, 0, False),       # 2^14 texels more
    (1 << 14, 1 << 14, 1, False),             # the same bitmap one texel further on
    (1 << 14, (1 << 14) - 1, 1 << 14, True),  # ends exactly at 2^28
    (1 << 14, (1 << 14) - 1, (1 << 14) + 1, False),
    (M24 - 1, 16, 0, True),                   # the widest side the 24-bit product takes: 2^28 - 16 texels
    (M24, 16, 0, False),                      # 2^28 texels, but a side of 2^24
    (M24, 1, 0, False),
    (16, M24 - 1, 0, True),
    (16, M24, 0, False),
    (1, M24, 0, False),
    (1, 1, M28 - 1, True),
    (1, 1, M28, False),
    (1, 1, 1 << 32, False),                   # an offset whose low word alone would pass
    (1, 1, (1 << 32) + 5, False),
    (65536, 65536, 0, False),                 # a product that wraps 32 bits to 0
]


@pytest.mark.parametrize("width,height,offset,on", _BITMAPS, ids=lambda v: str(v))
def test_the_route_is_on_exactly_inside_the_32_bit_addressing(lib, frame, width, height, offset, on):
    base = _cq(lib, frame)
    assert base > 0, "the scene's own frame takes the route"
    cq = _cq(lib, frame, width, height, offset)
    print(width, height, offset, cq)
    assert (offset + width * height <= M28 and width < M24 and height < M24) == on  # the table against the rule
    assert cq == (base if on else 0)


def _bits(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


_T = 800000.0
# (colour, power, lit + 4 * equal)
_LIGHTS = [
    ((1.0, 1.0, 1.0), _T, 7),
    ((0.5, 0.5, 0.5), 3.0, 7),
    ((1.0, 0.5, 0.25), _T, 3),
    ((1.0, 1.0, 0.99999994), _T, 3),          # one ulp apart
    ((1.0, 1.0, 0.0), _T, 3),
    ((0.0, 0.0, 0.0), _T, 6),                 # three +0: not lit, but bit-equal and every channel +0
    ((0.0, -0.0, 0.0), _T, 0),                # -0 is no +0: bit 1 fails, and `equal` with it
    ((-0.0, -0.0, -0.0), _T, 0),              # bit-equal, outside bit 1
    ((1e-19, 1e-19, 1e-19), 1.0, 1),          # bit-equal below 2^-60
    ((1.0, 1.0, 1.0), 1e19, 1),               # bit-equal above 2^60
    ((2.0 ** -60, 2.0 ** -60, 2.0 ** -60), 1.0, 7),
    ((-3.0, -3.0, -3.0), 1.0, 7),             # the window is on magnitudes
    ((float("inf"), float("inf"), float("inf")), 1.0, 1),
]


@pytest.mark.parametrize("color,power,lit", _LIGHTS, ids=lambda v: str(v))
def test_the_equal_channel_bit(lib, frame, color, power, lit):
    scene = frame[0]
    arr = (C.c_float * 3)(*color)
    got = lib.c2rt_light_lit_of(C.cast(scene.desc, C.c_void_p), arr, power)
    chans = [_bits(C.c_float(C.c_float(c).value * C.c_float(power).value).value) for c in color]
    print(color, power, ["%08x" % c for c in chans], got)
    assert got == lit
    # the rule, restated: equal = bit 1 and three equal bit patterns
    assert bool(got & 4) == (bool(got & 2) and chans[0] == chans[1] == chans[2])

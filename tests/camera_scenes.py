"""Cases for tests/test_camera_reference.py (CPU) and tests/test_gpu_camera.py: cameras with yaw, pitch AND roll, odd
frame sizes, stereo, depth of field, the pre-pass preview and interleaved strips, over the scenes of tests/geom_scenes.py
and tests/shade_scenes.py and one two-node scene of this file's own.  Every reference frame is computed once
(functools.lru_cache) by tests/camera_reference.py and is read-only.

  case             scene                        camera                                    frame    modes
  rolled           geom L1                      yaw 23.5, pitch -17, roll -7.25, fov 78   61x47    taps 1, 5, 4
  rolled_textured  shade L1 without its other   yaw -12, pitch -35, roll 11, fov 71       61x47    taps 1, 5
                   two planes and with the light
                   at y = 60 (bitmap floor, one
                   light: the ground path)
  tall             geom L2                      yaw 8, pitch -20, roll 3                  19x53    taps 5
  wide             floor and one sphere         rolled's                                  4099x9   taps 1
  stereo           geom L1                      rolled's, stereo_separation 0.5           37x29    taps 1, 5
  dof              shade L1                     rolled_textured's, depth of field:        24x17    taps 1, 5; seeds 7 and
                                                3 samples, fNumber 2, focal distance 42            (3 << 32) + 11
  dof_stereo       geom L1                      dof's lens, 2 samples, separation 0.5     24x17    taps 1
  preview          shade L1                     rolled_textured's; dof's lens             45x38    prepass_bucket 24: blocks of
                                                                                                   16 and 8, clipped by bucket
                                                                                                   and frame; lens off and on
  strips           shade L1                     dof's                                     24x23    strip_height 5, world 3:
                                                                                                   ranks 0, 1, 2 and the whole

The focal distance is about the floor's along the view axis (eye height 24 over sin 35 degrees).  `wide` has a width
that is no power of two and columns up to 4098: the reciprocal of the frame width is not exact."""
import functools
import os
import time

import numpy as np

import camera_reference as cr
import chess2rt_amd as c2
import geom_reference as gr
import geom_scenes as gs
import shade_reference as sr
import shade_scenes as ss
from chess2rt_amd import _abi

ROLLED = dict(yaw=23.5, pitch=-17.0, roll=-7.25, fov=78.0)
TEXTURED = dict(yaw=-12.0, pitch=-35.0, roll=11.0, fov=71.0)
TALL = dict(yaw=8.0, pitch=-20.0, roll=3.0)
LENS = dict(dof=True, num_samples=3, f_number=2.0, focal_plane_dist=42.0)
SEED_A, SEED_B = 7, (3 << 32) + 11
WIDE_W, WIDE_H = 4099, 9
WIDE_GROUND, WIDE_SPHERE = 0, 1


def _mode(name, taps=_abi.TAPS_1, seed=0, prepass_bucket=0, strip=None, **camera):
    """strip: (strip_height, strip_world, strip_rank); camera: what this mode changes in the case's camera"""
    return dict(name=name, taps=taps, seed=seed, prepass_bucket=prepass_bucket, strip=strip, camera=camera)


# case -> (scene, camera, W, H, modes)
CASES = {
    "rolled": (("geom", "L1"), ROLLED, 61, 47, [_mode("taps1"), _mode("taps5", _abi.TAPS_REF5), _mode("taps4", _abi.TAPS_4)]),
    "rolled_textured": (("shade_floor", "L1"), TEXTURED, 61, 47, [_mode("taps1"), _mode("taps5", _abi.TAPS_REF5)]),
    "tall": (("geom", "L2"), TALL, 19, 53, [_mode("taps5", _abi.TAPS_REF5)]),
    "wide": (("wide", None), ROLLED, WIDE_W, WIDE_H, [_mode("taps1")]),
    "stereo": (("geom", "L1"), dict(ROLLED, stereo_separation=0.5), 37, 29, [_mode("taps1"), _mode("taps5", _abi.TAPS_REF5)]),
    "dof": (("shade", "L1"), dict(TEXTURED, **LENS), 24, 17,
            [_mode("taps1_seedA", seed=SEED_A), _mode("taps5_seedA", _abi.TAPS_REF5, seed=SEED_A),
             _mode("taps1_seedB", seed=SEED_B), _mode("taps5_seedB", _abi.TAPS_REF5, seed=SEED_B)]),
    "dof_stereo": (("geom", "L1"), dict(ROLLED, **dict(LENS, num_samples=2, stereo_separation=0.5)), 24, 17, [_mode("taps1", seed=SEED_A)]),
    "preview": (("shade", "L1"), TEXTURED, 45, 38,
                [_mode("plain", prepass_bucket=24), _mode("lens", prepass_bucket=24, seed=SEED_A, **LENS)]),
    "strips": (("shade", "L1"), dict(TEXTURED, **LENS), 24, 23,
               [_mode("whole", seed=SEED_B)] + [_mode("rank%d" % r, seed=SEED_B, strip=(5, 3, r)) for r in range(3)]),
}
ALL = [(name, m["name"]) for name, c in CASES.items() for m in c[4]]
NO_LENS = [(name, m["name"]) for name, c in CASES.items() for m in c[4] if not dict(c[1], **m["camera"]).get("dof")]
IDS = ["%s-%s" % k for k in ALL]


def wide_text():
    """a floor and one sphere on the view axis of ROLLED from (5, 24, -72): no pow and no sin on the path"""
    return "\n".join([
        "Scene {", '  Name "camera_wide"',
        "  GlobalSettings { frameWidth %d; frameHeight %d; AAEnabled false; ambientLightColor 0.1 0.1 0.12 }" % (WIDE_W, WIDE_H),
        "  Camera { pos 5 24 -72; yaw 0; pitch -17; roll 0; fov 78 }",
        '  Lights {\n    PointLight "l0" { pos -30 60 -40; color 1 0.95 0.9; power 9000 }\n  }',
        '  Geometries {\n    Plane "ground" { y 0 }\n    Sphere "ball" { center %r %r %r; R 9 }\n  }' % WIDE_BALL,
        '  Textures {\n    Checker "chk" { color1 0.9 0.1 0.2; color2 0.15 0.8 0.95; size 3.5 }\n  }',
        '  Shaders {\n    Lambert "sh_ground" { texture "chk" }\n    Lambert "sh_ball" { color 0.3 0.7 0.4 }\n  }',
        '  Nodes {\n    Node "n0" { geometry "ground"; shader "sh_ground" }\n    Node "n1" { geometry "ball"; shader "sh_ball" }\n  }',
        "}", ""])


WIDE_BALL = (-12.0, 12.0, -33.0)


class Mode:
    """name, taps, seed | params: begin_frame's arguments | frame: cr.Frame | cam: that frame as a c2rt_camera_frame |
    host_cam: the host mirror's beginFrame for the same camera | opts: c2rt_render_opts | ropts: cr.Opts"""


class Case:
    """name, W, H | scene: the loaded scene (this case's own) | desc | tables: (gr.Tables, sr.Tables) | modes: name -> Mode"""


def to_abi(frame):
    cam = _abi.CameraFrame()
    for f in cr.FRAME_VECTORS:
        getattr(cam, f)[:] = [float(v) for v in getattr(frame, f)]
    cam.frame_width, cam.frame_height = float(frame.frame_width), float(frame.frame_height)
    cam.dof, cam.num_samples = int(frame.dof), int(frame.num_samples)
    cam.focal_plane_dist, cam.disc_multiplier = float(frame.focal_plane_dist), float(frame.disc_multiplier)
    cam.stereo_separation = float(frame.stereo_separation)
    return cam


def from_abi(cam, f_number=None):
    """a c2rt_camera_frame as a cr.Frame (f_number, which only a mutation reads, from disc_multiplier unless given)"""
    fr = cr.Frame()
    for f in cr.FRAME_VECTORS:
        setattr(fr, f, np.array(list(getattr(cam, f)), dtype=np.float64))
    fr.frame_width, fr.frame_height = np.float64(cam.frame_width), np.float64(cam.frame_height)
    fr.dof, fr.num_samples = bool(cam.dof), int(cam.num_samples)
    fr.focal_plane_dist, fr.disc_multiplier = np.float64(cam.focal_plane_dist), np.float64(cam.disc_multiplier)
    fr.f_number = np.float64(f_number if f_number is not None else 10.0 / cam.disc_multiplier)
    fr.stereo_separation = np.float64(cam.stereo_separation)
    return fr


def frame_bits(cam):
    """the seven vectors, the frame size and the lens fields of a c2rt_camera_frame or a cr.Frame, as one tuple of bits"""
    out = []
    for f in cr.FRAME_VECTORS:
        out += [np.float64(v).view(np.uint64) for v in getattr(cam, f)]
    for f in ("frame_width", "frame_height", "focal_plane_dist", "disc_multiplier", "stereo_separation"):
        out.append(np.float64(getattr(cam, f)).view(np.uint64))
    return tuple(int(v) for v in out) + (int(cam.dof), int(cam.num_samples))


def host_camera(scene, W, H, **params):
    """sets the loaded scene's camera through scene.camera and returns (begin_frame's arguments, the host's beginFrame)"""
    scene.setFrameSize(W, H)
    hc = scene.camera
    for k, v in params.items():
        setattr(hc, k, v)
    hc.disc_multiplier = 10.0 / hc.f_number                 # what deserialize leaves (rt/camera.d:252)
    scene.camera = hc
    cam = scene.beginFrame()
    hc = scene.camera
    args = dict(pos=tuple(hc.pos), yaw=hc.yaw, pitch=hc.pitch, roll=hc.roll, fov=hc.fov, W=W, H=H, dof=bool(hc.dof),
                num_samples=int(hc.num_samples), focal_plane_dist=hc.focal_plane_dist, f_number=hc.f_number,
                stereo_separation=hc.stereo_separation)
    return args, cam


def _load(kind, variant, tag):
    if kind == "geom":
        g = gs.load(variant, tag)
        return g.scene, g.desc, g
    if kind in ("shade", "shade_floor"):
        scene = ss.load(variant, False, tag, kind == "shade_floor")[0]
        return scene, scene.desc.contents, scene
    path = os.path.join(ss._TMP, "camera_wide.sdl")
    with open(path, "w") as f:
        f.write(wide_text())
    scene = c2.parseSceneFromFile(path)
    return scene, scene.desc.contents, scene


@functools.lru_cache(maxsize=None)
def case(name):
    (kind, variant), camera, W, H, modes = CASES[name]
    c = Case()
    c.name, c.W, c.H = name, W, H
    c.scene, c.desc, c._keep = _load(kind, variant, "camera_" + name)
    c.scene.setAA(False)
    c.tables = (gr.Tables(c.desc), sr.Tables(c.desc))
    c.modes = {}
    for m in modes:
        o = Mode()
        o.name, o.taps, o.seed = m["name"], m["taps"], m["seed"]
        reset = dict(dof=0, stereo_separation=0.0)
        o.params, o.host_cam = host_camera(c.scene, W, H, **dict(reset, **dict(camera, **m["camera"])))
        o.frame = cr.begin_frame(**o.params)
        o.cam = to_abi(o.frame)
        kw = dict(taps=m["taps"], seed=m["seed"], prepass_bucket=m["prepass_bucket"])
        if m["strip"]:
            kw.update(strip_height=m["strip"][0], strip_world=m["strip"][1], strip_rank=m["strip"][2])
        o.opts = c.scene.renderOpts(**kw)
        o.ropts = cr.Opts(W, H, **kw)
        c.modes[o.name] = o
    return c


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """cr.render_frame of one case and mode, once; `seconds` is what it took"""
    c = case(name)
    m = c.modes[mode]
    t0 = time.time()
    r = cr.render_frame(c.tables, m.frame, m.ropts)
    r.seconds = time.time() - t0
    for a in (r.rgb, r.lo, r.hi, r.ambiguous, r.wide, r.rays):
        a.setflags(write=False)
    return r


def ambiguity_cap(r):
    """the share of pixels held to an interval may be at most 0.001 per sample of a pixel"""
    return r.samples_per_pixel * 0.001


def pixel_rays(name, mode="taps1"):
    """(W * H, 6): the reference's ray of every integer pixel of a one-tap mode without a lens, row-major"""
    c = case(name)
    yy, xx = np.meshgrid(np.arange(c.H), np.arange(c.W), indexing="ij")
    o, d = cr.screen_ray(c.modes[mode].frame, xx.ravel(), yy.ravel())
    return np.ascontiguousarray(np.hstack([o, d]))


def encode_rgb32(rgb):
    """the host's display encoding (Color.toRGB32) of every pixel of a float frame -> uint32 of the frame's shape"""
    lib = _abi.load_library()
    flat = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1, 3)
    out = np.array([lib.c2rt_host_color_to_rgb32(px.ctypes.data_as(_abi._f32p)) for px in flat], dtype=np.uint32)
    return out.reshape(np.shape(rgb)[:-1])


def probed_ray(name, mode, x, y):
    """(6,): the ray renderPixel(x, y) reports — the LAST lens sample's (the probe is overwritten per sample), the left
    eye's under stereo (rt/renderer.d:46-57 traces one ray; the build keeps the first eye's)"""
    c = case(name)
    r = reference(name, mode)
    fr = c.modes[mode].frame
    ne = 2 if fr.stereo_separation != 0 else 1
    ns = fr.num_samples if fr.dof else 1
    per_tap = r.rays[: ns * ne * c.W * c.H].reshape(ns, ne, c.H * c.W, 6)
    return per_tap[ns - 1, 0, y * c.W + x]


def probe_pixels(W, H, n=64, seed=41):
    """the four corners, both edges' midpoints, the centre and seeded random pixels: n of them, distinct"""
    fixed = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2), (W // 2, H // 2)]
    rng = np.random.RandomState(seed)
    out = list(dict.fromkeys(fixed))
    while len(out) < n:
        p = (int(rng.randint(W)), int(rng.randint(H)))
        if p not in out:
            out.append(p)
    return out[:n]

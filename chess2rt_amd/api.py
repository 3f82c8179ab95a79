"""Python face of the Chess2RT GPU render path.

Thin wrappers over the C ABI (include/c2rt.h) and the C++ host mirror
(include/c2rt_host.h) that keep the reference's names: ``parseSceneFromFile``
(rt/scene_loader.d:20-41), ``Scene.beginFrame`` (rt/scene.d:55-58),
``Renderer.renderRT`` / ``renderPixelNoAA`` (rt/renderer.d:83,223),
``renderPixel`` (rt/renderer.d:46-57).  Python holds no algorithm: all
rendering happens in libc2rt.so on the GPU.  The hit, shading, occlusion, gather
and path planes are each described once (``_PlaneFamily``: struct, table, noun).
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import (CameraFrame, DenoiseGuides, DenoiseOpts, DenoiseVarianceOpts, GatherOpts, GatherPlanes, HitPlanes, HostCamera, HostSettings, OcclusionOpts, OcclusionPlanes, PathCountOpts, PathOpts, PathPlanes, Ray, RayHit, RayStats, RenderOpts, SceneDesc,
                   ScenePose, Segment, ShadePlanes, TapTable, TemporalGuides, TemporalMotion, TemporalOpts, TemporalPlanes, TraceResult)

# c2rt_ray_hit as a structured numpy dtype (the layout of _abi.RayHit / include/c2rt.h: 80 bytes)
RAY_HIT_DTYPE = np.dtype({
    "names": ["closest_node", "leaf_geom", "dist", "u", "v", "p", "normal"],
    "formats": [np.int32, np.int32, np.float64, np.float64, np.float64, (np.float64, 3), (np.float64, 3)],
    "offsets": [RayHit.closest_node.offset, RayHit.leaf_geom.offset, RayHit.dist.offset, RayHit.u.offset, RayHit.v.offset,
                RayHit.p.offset, RayHit.normal.offset],
    "itemsize": C.sizeof(RayHit),
})


class _PlaneFamily:
    """One plane family, described once: the ctypes struct of its pointers, its table {plane name: (dtype, components
    per sample)} in the order of the struct's members, and the noun its ValueError names it by."""

    def __init__(self, struct, table, noun):
        self.struct, self.table, self.noun = struct, table, noun

    def _known(self, n):
        if n not in self.table:
            raise ValueError("unknown %s plane %r (one of %s)" % (self.noun, n, ", ".join(self.table)))

    def new(self, names, shape):
        """(struct of fresh host arrays, {name: array}) for the planes named, `shape` samples each; the others stay null"""
        names = tuple(names)
        for n in names:
            self._known(n)
        out, pl = {}, self.struct()
        for n in names:
            dtype, comps = self.table[n]
            out[n] = np.empty(tuple(shape) if comps == 1 else tuple(shape) + (comps,), dtype=dtype)
            setattr(pl, n, out[n].ctypes.data)
        return pl, out

    def device(self, ptrs):
        """struct of the device pointers in `ptrs` ({plane name: pointer}); planes left out (or 0 / None) stay null"""
        pl = self.struct()
        for n, ptr in dict(ptrs).items():
            self._known(n)
            setattr(pl, n, ptr or None)
        return pl


# c2rt_hit_planes: plane name -> (dtype, components per pixel), in the order of the struct's members
HIT_PLANES = {"node": (np.int32, 1), "leaf": (np.int32, 1), "dist": (np.float64, 1), "uv": (np.float64, 2),
              "p": (np.float64, 3), "normal": (np.float64, 3), "rgb": (np.float32, 3)}
# c2rt_shade_planes: plane name -> (dtype, components per sample), in the order of the struct's members
SHADE_PLANES = {"node": (np.int32, 1), "albedo": (np.float32, 3), "light": (np.float32, 3), "specular": (np.float32, 3),
                "visible": (np.uint32, 1), "rgb": (np.float32, 3)}
# c2rt_occlusion_planes: plane name -> (dtype, components per sample), in the order of the struct's members
OCCLUSION_PLANES = {"node": (np.int32, 1), "open": (np.uint64, 1), "ao": (np.float32, 1), "bent": (np.float64, 3)}
# c2rt_gather_planes: plane name -> (dtype, components per sample), in the order of the struct's members
GATHER_PLANES = {"node": (np.int32, 1), "hits": (np.uint64, 1), "indirect": (np.float32, 3), "bounce": (np.float32, 3)}
# c2rt_path_planes: plane name -> (dtype, components per sample), in the order of the struct's members
PATH_PLANES = {"node": (np.int32, 1), "segments": (np.uint32, 1), "indirect": (np.float32, 3), "bounce": (np.float32, 3), "radiance": (np.float32, 3)}

_HIT = _PlaneFamily(HitPlanes, HIT_PLANES, "hit")
_SHADE = _PlaneFamily(ShadePlanes, SHADE_PLANES, "shading")
_OCCLUSION = _PlaneFamily(OcclusionPlanes, OCCLUSION_PLANES, "occlusion")
_GATHER = _PlaneFamily(GatherPlanes, GATHER_PLANES, "gather")
_PATHS = _PlaneFamily(PathPlanes, PATH_PLANES, "path")


def _rays_array(rays, what="rays"):
    """`rays` (c2rt_ray: origin, direction; c2rt_segment: from, to) as a contiguous (n, 6) float64 array"""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    if rays.ndim != 2 or rays.shape[1] != 6:
        raise ValueError("%s: expected shape (n, 6), got %r" % (what, rays.shape))
    return rays


def _occlusion_opts(samples, radius, seed):
    return OcclusionOpts(radius=float(radius), seed=int(seed), samples=int(samples), reserved=0)


# the reference's five taps (rt/renderer.d:235-242): the table behind C2RT_TAPS_REF5, its first four behind C2RT_TAPS_4
TAPS_REF5_TABLE = ((0.0, 0.0), (0.3, 0.3), (0.6, 0.0), (0.0, 0.6), (0.6, 0.6))


def tap_grid(k):
    """The k x k regular grid (1 <= k <= 4) as a tuple of (dx, dy): tap s at ((s % k) / k, (s // k) / k), so tap 0 is
    the pixel's corner (0, 0) and the table also serves the adaptive calls."""
    if not 1 <= k <= 4:
        raise ValueError("tap_grid: k is %r (1 .. 4: at most %d taps)" % (k, _abi.MAX_SAMPLE_TAPS))
    return tuple((float(s % k) / float(k), float(s // k) / float(k)) for s in range(k * k))


def _tap_table(taps):
    """c2rt_tap_table of a TapTable (as it is) or of a sequence of (dx, dy); a sequence longer than the struct holds
    keeps its count, which the library refuses"""
    if isinstance(taps, TapTable):
        return taps
    taps = list(taps)
    t = TapTable()
    t.n = len(taps)
    for s, (dx, dy) in enumerate(taps[:_abi.MAX_SAMPLE_TAPS]):
        t.offset[s][0] = dx
        t.offset[s][1] = dy
    return t


def _gather_opts(samples, seed):
    return GatherOpts(seed=int(seed), samples=int(samples), reserved=0)


def _path_opts(paths, bounces, seed):
    return PathOpts(seed=int(seed), paths=int(paths), bounces=int(bounces))


# Context.denoise's sigma_plane when none is given: a tap one world unit off the centre's tangent plane weighs half
DENOISE_SIGMA_PLANE = 1.0


def _denoise_opts(width, height, channels, levels, normal_power_log2, sigma_plane, sigma_colour):
    return DenoiseOpts(width=int(width), height=int(height), levels=int(levels), channels=int(channels), normal_power_log2=int(normal_power_log2),
                       sigma_plane=float(sigma_plane), sigma_colour=float(sigma_colour), reserved=0)


def denoise_scratch_bytes(width, height, channels=3, levels=5, normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE, sigma_colour=0.0):
    """c2rt_denoise_scratch_bytes: what Context.denoiseDevice needs at `scratch_ptr` for these options (the guides packed
    to fp32, 32 B per pixel, and for levels > 1 one ping-pong plane); 0 for levels == 0 and for options it would refuse."""
    o = _denoise_opts(width, height, channels, levels, normal_power_log2, sigma_plane, sigma_colour)
    return int(_abi.load_library().c2rt_denoise_scratch_bytes(C.byref(o)))


# Context.denoiseVariance's luminance scale (a tap whose luminance differs by sigma_lum local standard deviations weighs
# half), the floor under the scaled variance, and the age below which a pixel's variance is estimated from its 7x7
DENOISE_SIGMA_LUM = 4.0
DENOISE_VAR_FLOOR = 1e-8
DENOISE_MIN_AGE = 4


def _denoise_variance_opts(width, height, channels, levels, normal_power_log2, sigma_plane, sigma_lum, var_floor, min_age):
    return DenoiseVarianceOpts(width=int(width), height=int(height), levels=int(levels), channels=int(channels), normal_power_log2=int(normal_power_log2),
                               sigma_plane=float(sigma_plane), sigma_lum=float(sigma_lum), var_floor=float(var_floor), min_age=int(min_age), reserved=0)


def denoise_variance_scratch_bytes(width, height, channels=3, levels=5, normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE, sigma_lum=DENOISE_SIGMA_LUM,
                                   var_floor=DENOISE_VAR_FLOOR, min_age=DENOISE_MIN_AGE):
    """c2rt_denoise_variance_scratch_bytes: what Context.denoiseVarianceDevice needs at `scratch_ptr` for these options
    (the packed guides, the colour ping-pong plane, three variance planes: at most 56 B per pixel); 0 for refused options."""
    o = _denoise_variance_opts(width, height, channels, levels, normal_power_log2, sigma_plane, sigma_lum, var_floor, min_age)
    return int(_abi.load_library().c2rt_denoise_variance_scratch_bytes(C.byref(o)))


# Context.temporalAccumulate's defaults: the running mean grows to 32 samples; a history tap counts within 25 degrees of
# the pixel's normal and a tenth of a world unit of its tangent plane
TEMPORAL_MAX_AGE = 32
TEMPORAL_MIN_NORMAL_DOT = 0.9
TEMPORAL_MAX_PLANE_DIST = 0.1
# c2rt_temporal_planes: plane name -> dtype ("colour" has the input's channels, the others one value per pixel)
TEMPORAL_PLANES = {"colour": np.float32, "variance": np.float32, "age": np.uint32}
# Context.pathCounts' defaults: 2 .. 64 paths, 16 where the history is missing or younger than 2 samples, and 2000 paths
# per unit of per-path luminance variance
PATH_COUNT_MIN = 2
PATH_COUNT_MAX = 64
PATH_COUNT_YOUNG = 16
PATH_COUNT_MIN_AGE = 2
PATH_COUNT_PER_VARIANCE = 2000.0


def _temporal_opts(width, height, channels, max_age, min_normal_dot, max_plane_dist):
    return TemporalOpts(width=int(width), height=int(height), channels=int(channels), max_age=int(max_age), min_normal_dot=float(min_normal_dot),
                        max_plane_dist=float(max_plane_dist))


def temporal_history_bytes(width, height, channels=3, max_age=TEMPORAL_MAX_AGE, min_normal_dot=TEMPORAL_MIN_NORMAL_DOT,
                           max_plane_dist=TEMPORAL_MAX_PLANE_DIST):
    """c2rt_temporal_history_bytes: the size of one history of Context.temporalAccumulate / temporalAccumulateDevice,
    width * height * (32 + 4 * channels + 8); 0 for options the library would refuse."""
    o = _temporal_opts(width, height, channels, max_age, min_normal_dot, max_plane_dist)
    return int(_abi.load_library().c2rt_temporal_history_bytes(C.byref(o)))


def _path_count_opts(min_paths, max_paths, young_paths, min_age, paths_per_variance, prev_paths):
    return PathCountOpts(min_paths=min_paths, max_paths=max_paths, young_paths=young_paths, min_age=min_age, paths_per_variance=paths_per_variance,
                         prev_paths=prev_paths)


def paths_counted_scratch_bytes(n_samples):
    """Bytes of the count-order scratch of the counted path planes' device calls for `n_samples` samples
    (c2rt_paths_counted_scratch_bytes: 512 + 4 * n_samples rounded up to 16; no context)"""
    return int(_abi.load_library().c2rt_paths_counted_scratch_bytes(int(n_samples)))


def _counts_array(counts, shape, what):
    counts = np.ascontiguousarray(counts, dtype=np.uint8)
    if counts.shape != tuple(shape):
        raise ValueError("%s: counts of shape %r (expected %r)" % (what, counts.shape, tuple(shape)))
    return counts


def makeMotion(motion):
    """c2rt_temporal_motion from ``motion = {node index: (prev, cur)}``: for every node that moved, the transform the
    history was made under and the transform of the current guides (30 doubles each, as for makePose).  A TemporalMotion
    passes through.  Entries keep the order of the dict.  The arrays live as long as the TemporalMotion returned."""
    if isinstance(motion, TemporalMotion):
        return motion
    motion = dict(motion)
    m = TemporalMotion()
    if motion:
        idx = np.array(list(motion), dtype=np.uint32)
        prev = np.ascontiguousarray([np.asarray(v[0], dtype=np.float64).reshape(30) for v in motion.values()])
        cur = np.ascontiguousarray([np.asarray(v[1], dtype=np.float64).reshape(30) for v in motion.values()])
        m.n_nodes = len(idx)
        m.node_index = idx.ctypes.data_as(_abi._u32p)
        m.prev_transform = prev.ctypes.data_as(_abi._f64p)
        m.cur_transform = cur.ctypes.data_as(_abi._f64p)
        m._keep = [idx, prev, cur]
    return m


def makePose(nodes=None, lights=None):
    """c2rt_scene_pose from ``nodes = {index: transform}`` (30 doubles each, the layout of SceneDesc.node_transform:
    transform, inverseTransform, transposedInverse, offset) and ``lights = {index: dict(pos=, color=, power=)}``.  The
    light arrays of a pose are per pose, not per light: every light listed gives the same keys.  Entries keep the
    order of the dicts.  The arrays live as long as the ScenePose returned."""
    nodes, lights = dict(nodes or {}), dict(lights or {})
    pose = ScenePose()
    keep = []
    if nodes:
        idx = np.array(list(nodes), dtype=np.uint32)
        xf = np.ascontiguousarray([np.asarray(t, dtype=np.float64).reshape(30) for t in nodes.values()])
        pose.n_nodes = len(idx)
        pose.node_index = idx.ctypes.data_as(_abi._u32p)
        pose.node_transform = xf.ctypes.data_as(_abi._f64p)
        keep += [idx, xf]
    if lights:
        keys = {tuple(sorted(v)) for v in lights.values()}
        if len(keys) != 1 or not set(next(iter(keys))) <= {"pos", "color", "power"}:
            raise ValueError("lights: every entry gives the same keys out of pos, color, power")
        idx = np.array(list(lights), dtype=np.uint32)
        pose.n_lights = len(idx)
        pose.light_index = idx.ctypes.data_as(_abi._u32p)
        keep.append(idx)
        for key, field, dtype, ptr in (("pos", "light_pos", np.float64, _abi._f64p), ("color", "light_color", np.float32, _abi._f32p),
                                       ("power", "light_power", np.float32, _abi._f32p)):
            if key in next(iter(keys)):
                a = np.ascontiguousarray([np.asarray(v[key], dtype=dtype).reshape(-1) for v in lights.values()])
                setattr(pose, field, a.ctypes.data_as(ptr))
                keep.append(a)
    pose._keep = keep
    return pose


class C2rtError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("c2rt status %d (%s): %s" % (status, _status_string(status), message))
        self.status = status


def _status_string(status):
    return _abi.load_library().c2rt_status_string(status).decode()


class Scene:
    """Host-side scene (mirror of rt/scene.d Scene), loaded from .sdl/.json."""

    def __init__(self, handle):
        self._lib = _abi.load_library()
        self._h = C.c_void_p(handle)

    def close(self):
        if self._h:
            self._lib.c2rt_host_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def name(self):
        return self._lib.c2rt_host_scene_name(self._h).decode()

    @property
    def settings(self):
        s = HostSettings()
        self._lib.c2rt_host_scene_get_settings(self._h, C.byref(s))
        return s

    @property
    def camera(self):
        c = HostCamera()
        self._lib.c2rt_host_scene_get_camera(self._h, C.byref(c))
        return c

    @camera.setter
    def camera(self, cam):
        self._lib.c2rt_host_scene_set_camera(self._h, C.byref(cam))

    @property
    def desc(self):
        """POINTER(SceneDesc): the flat tables (owned by the scene)."""
        return self._lib.c2rt_host_scene_desc(self._h)

    def setFrameSize(self, width, height):
        """RTDemo.updateToWindowSize (gui/raytracer_demo.d:126-143)."""
        self._lib.c2rt_host_scene_set_frame_size(self._h, int(width), int(height))

    def setAA(self, enabled):
        self._lib.c2rt_host_scene_set_aa(self._h, 1 if enabled else 0)

    def setDof(self, enabled):
        self._lib.c2rt_host_scene_set_dof(self._h, 1 if enabled else 0)

    def beginFrame(self):
        cam = CameraFrame()
        self._lib.c2rt_host_scene_begin_frame(self._h, C.byref(cam))
        return cam

    def moveCamera(self, dx, dy, dz):
        self._lib.c2rt_host_camera_move(self._h, dx, dy, dz)

    def rotateCamera(self, dyaw, droll, dpitch):
        self._lib.c2rt_host_camera_rotate(self._h, dyaw, droll, dpitch)

    def nodeIndex(self, name):
        """index of the named node in the flat tables (and in a c2rt_scene_pose); -1: no such node"""
        return int(self._lib.c2rt_host_scene_node_index(self._h, name.encode()))

    def lightIndex(self, name):
        return int(self._lib.c2rt_host_scene_light_index(self._h, name.encode()))

    def nodeTransform(self, name):
        """the named node's Transform as 30 doubles (transform, inverseTransform, transposedInverse, offset): edit it with
        the c2rt_host_transform_* calls (rt/transform.d's scale / rotate / translate / reset) and hand it back"""
        t = np.empty(30, dtype=np.float64)
        if self._lib.c2rt_host_node_transform_get(self._h, name.encode(), t.ctypes.data_as(_abi._f64p)) != _abi.OK:
            raise KeyError(name)
        return t

    def setNodeTransform(self, name, transform, ctx=None):
        """Sets the named node's Transform on the host object; with `ctx`, and if that context still holds this scene's
        upload, also pushes the change to it (one c2rt_update_scene, on the default stream); otherwise the next render
        through a Renderer re-uploads."""
        t = np.ascontiguousarray(transform, dtype=np.float64).reshape(30)
        st = self._lib.c2rt_host_node_transform_set(ctx.handle if ctx is not None else None, self._h, name.encode(),
                                                          t.ctypes.data_as(_abi._f64p))
        if st != _abi.OK:
            raise C2rtError(st, ctx._lib.c2rt_last_error(ctx.handle).decode(errors="replace") if ctx is not None and st != _abi.ERR_INVALID_ARG
                            else "no node named %r" % name)

    def _node_verb(self, fn, name, ctx, *args):
        st = fn(ctx.handle if ctx is not None else None, self._h, name.encode(), *args)
        if st != _abi.OK:
            raise C2rtError(st, ctx._lib.c2rt_last_error(ctx.handle).decode(errors="replace") if ctx is not None and st != _abi.ERR_INVALID_ARG
                            else "no node named %r" % name)

    def resetNode(self, name, ctx=None):
        """Transform.reset (rt/transform.d:24-29) on the named node; `ctx` as in setNodeTransform"""
        self._node_verb(self._lib.c2rt_host_node_transform_reset, name, ctx)

    def scaleNode(self, name, x, y, z, ctx=None):
        self._node_verb(self._lib.c2rt_host_node_transform_scale, name, ctx, x, y, z)

    def rotateNode(self, name, yaw, pitch, roll, ctx=None):
        self._node_verb(self._lib.c2rt_host_node_transform_rotate, name, ctx, yaw, pitch, roll)

    def translateNode(self, name, v, ctx=None):
        self._node_verb(self._lib.c2rt_host_node_transform_translate, name, ctx, (C.c_double * 3)(*v))

    def setLight(self, name, pos=None, color=None, power=None, ctx=None):
        """Sets the named light's position, colour and power (None: unchanged); `ctx` as in setNodeTransform."""
        p = np.ascontiguousarray(pos, dtype=np.float64).reshape(3) if pos is not None else None
        c = np.ascontiguousarray(color, dtype=np.float32).reshape(3) if color is not None else None
        w = np.array([power], dtype=np.float32) if power is not None else None
        st = self._lib.c2rt_host_light_set(ctx.handle if ctx is not None else None, self._h, name.encode(),
                                                 p.ctypes.data_as(_abi._f64p) if p is not None else None,
                                                 c.ctypes.data_as(_abi._f32p) if c is not None else None,
                                                 w.ctypes.data_as(_abi._f32p) if w is not None else None)
        if st != _abi.OK:
            raise C2rtError(st, ctx._lib.c2rt_last_error(ctx.handle).decode(errors="replace") if ctx is not None and st != _abi.ERR_INVALID_ARG
                            else "no light named %r" % name)

    def renderOpts(self, **kw):
        s = self.settings
        o = RenderOpts()
        o.width, o.height = s.frame_width, s.frame_height
        o.taps = _abi.TAPS_REF5 if s.aa_enabled else _abi.TAPS_1
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def parseSceneFromFile(path):
    lib = _abi.load_library()
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    st = lib.c2rt_host_scene_load(str(path).encode(), C.byref(h), err, len(err))
    if st != _abi.OK:
        raise C2rtError(st, err.value.decode(errors="replace"))
    return Scene(h.value)


class Context:
    """One GPU context (c2rt_ctx).  Raises if no GPU is usable.

    ``Context(device)``: one device (c2rt_init).  ``Context(devices=[...])``: ONE context over several
    device slots of this process (c2rt_init_multi; ids may repeat, ``devices=0`` = every visible GPU):
    host-output frames are dealt to the slots in interleaved strips, device-output frames are stored by
    every slot straight into the lead device's frame."""

    def __init__(self, device=-1, devices=None):
        self._lib = _abi.load_library()
        h = C.c_void_p()
        if devices is None:
            st = self._lib.c2rt_init(int(device), C.byref(h))
        elif isinstance(devices, int):
            st = self._lib.c2rt_init_multi(int(devices), None, C.byref(h))
        else:
            ids = (C.c_int * len(devices))(*[int(d) for d in devices])
            st = self._lib.c2rt_init_multi(len(devices), ids, C.byref(h))
        self._h = h if h.value else None
        if st != _abi.OK:
            msg = self._lib.c2rt_last_error(self._h).decode() if self._h else ""
            if self._h:
                self._lib.c2rt_destroy(self._h)
                self._h = None
            raise C2rtError(st, msg)

    def close(self):
        if self._h:
            self._lib.c2rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _check(self, st):
        if st != _abi.OK:
            raise C2rtError(st, self._lib.c2rt_last_error(self._h).decode(errors="replace"))

    @property
    def deviceCount(self):
        return int(self._lib.c2rt_device_count(self._h))

    @property
    def sceneGeneration(self):
        return int(self._lib.c2rt_scene_generation(self._h))

    def uploadScene(self, desc):
        """desc: POINTER(SceneDesc) or SceneDesc."""
        if isinstance(desc, SceneDesc):
            desc = C.pointer(desc)
        self._check(self._lib.c2rt_upload_scene(self._h, desc))

    def updateScene(self, nodes=None, lights=None, stream=None):
        """Moves nodes and lights of the uploaded scene without re-uploading it (c2rt_update_scene): ``nodes = {index:
        transform}`` (30 doubles, see makePose), ``lights = {index: dict(pos=, color=, power=)}``.  The table copies are
        ordered on `stream` (None: the default stream): frames enqueued there before the call see the old scene, frames
        after it the new one, with no sync in between.  The context then behaves as after a fresh upload of the patched
        description; sceneGeneration does not change."""
        self.updateScenePose(makePose(nodes, lights), stream)

    def updateScenePose(self, pose, stream=None):
        self._check(self._lib.c2rt_update_scene(self._h, C.byref(pose), C.c_void_p(stream or None)))

    @staticmethod
    def _pose_array(poses):
        """(contiguous ctypes array, count, what keeps its arrays alive) of a sequence of ScenePose or (nodes, lights) pairs"""
        if isinstance(poses, C.Array):
            return poses, len(poses), None
        poses = [p if isinstance(p, ScenePose) else makePose(*p) for p in poses]
        return (ScenePose * max(len(poses), 1))(*poses), len(poses), poses

    def _posed_arrays(self, cams, poses):
        """(camera array, pose array, count, what keeps the poses' arrays alive) of a posed batch: n cameras, n poses"""
        arr, n = self._camera_array(cams)
        parr, np_, keep = self._pose_array(poses)
        if np_ != n:
            raise ValueError("%d cameras, %d poses" % (n, np_))
        return arr, parr, n, keep

    def renderFramesPosed(self, cams, poses, opts, stop_flag=None):
        """An animation in one call (c2rt_render_frames_posed): frame i is the current scene with poses[i] applied — a
        ScenePose or a (nodes, lights) pair as for updateScene, each relative to the current scene — seen through
        cams[i]: the bits of updateScene(poses[i]) + renderFrame(cams[i]).  The context's scene is unchanged.  A new
        host array of shape (len(cams), local_rows, W, 3)."""
        arr, parr, n, keep = self._posed_arrays(cams, poses)
        out = np.empty((n, self.localRows(opts), opts.width, 3), dtype=np.float32)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self._check(self._lib.c2rt_render_frames_posed(self._h, arr, parr, n, C.byref(opts), out.ctypes.data_as(C.c_void_p), stop))
        return out

    def renderFramesPosedDevice(self, cams, poses, opts, out_ptr, stream=0):
        """Enqueue the posed batch into device memory (len(cams) * local_rows * W * 3 floats at out_ptr) on `stream`."""
        arr, parr, n, keep = self._posed_arrays(cams, poses)
        self._check(self._lib.c2rt_render_frames_posed_device(self._h, arr, parr, n, C.byref(opts), C.c_void_p(out_ptr), C.c_void_p(stream)))

    def localRows(self, opts):
        return int(self._lib.c2rt_local_rows(C.byref(opts)))

    def renderFrame(self, cam, opts, stop_flag=None):
        """Blocking render into a new host array of shape (local_rows, W, 3)."""
        rows = self.localRows(opts)
        out = np.empty((rows, opts.width, 3), dtype=np.float32)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self._check(self._lib.c2rt_render_frame(self._h, C.byref(cam), C.byref(opts), out.ctypes.data_as(C.c_void_p), stop))
        return out

    def renderFrameInto(self, cam, opts, out, stop_flag=None):
        """Blocking render into a caller-owned float32 array (e.g. one pinned with pinHostBuffer)."""
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.size >= self.localRows(opts) * opts.width * 3
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self._check(self._lib.c2rt_render_frame(self._h, C.byref(cam), C.byref(opts), out.ctypes.data_as(C.c_void_p), stop))
        return out

    def pinHostBuffer(self, arr):
        self._check(self._lib.c2rt_pin_host_buffer(self._h, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def unpinHostBuffer(self, arr):
        self._check(self._lib.c2rt_unpin_host_buffer(self._h, arr.ctypes.data_as(C.c_void_p)))

    def renderFrameDevice(self, cam, opts, out_ptr, stream=0):
        """Enqueue a render into device memory (e.g. tensor.data_ptr())."""
        self._check(self._lib.c2rt_render_frame_device(self._h, C.byref(cam), C.byref(opts), C.c_void_p(out_ptr), C.c_void_p(stream)))

    @staticmethod
    def _camera_array(cams):
        """(contiguous ctypes array, count) of a sequence of CameraFrame or of a ctypes array of them"""
        if isinstance(cams, C.Array):
            return cams, len(cams)
        cams = list(cams)
        return (CameraFrame * max(len(cams), 1))(*cams), len(cams)

    def renderFrames(self, cams, opts, stop_flag=None):
        """One call for a batch of cameras of the uploaded scene (c2rt_render_frames): a new host array of shape
        (len(cams), local_rows, W, 3); frame i holds the bits renderFrame(cams[i], opts) returns.  No depth of field,
        stereo, count_rays or prepass_bucket in a batch (C2rtError, status ERR_UNSUPPORTED)."""
        arr, n = self._camera_array(cams)
        out = np.empty((n, self.localRows(opts), opts.width, 3), dtype=np.float32)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self._check(self._lib.c2rt_render_frames(self._h, arr, n, C.byref(opts), out.ctypes.data_as(C.c_void_p), stop))
        return out

    def renderFramesDevice(self, cams, opts, out_ptr, stream=0):
        """Enqueue the batch into device memory (len(cams) * local_rows * W * 3 floats at out_ptr) on `stream`."""
        arr, n = self._camera_array(cams)
        self._check(self._lib.c2rt_render_frames_device(self._h, arr, n, C.byref(opts), C.c_void_p(out_ptr), C.c_void_p(stream)))

    def renderFrameAdaptive(self, cam, opts, threshold=_abi.AA_THRESHOLD_REF, stop_flag=None):
        """Adaptive anti-aliasing (c2rt_render_frame_adaptive; opts.taps must be TAPS_REF5): (frame, mask) — the
        (H, W, 3) float32 frame and the (H, W) uint8 flags of the reference's edge test at `threshold`.  A flagged pixel
        holds the bits of the five-tap frame, an unflagged one the bits of the one-tap frame.  No depth of field, stereo,
        count_rays, prepass_bucket, strips or multi-device context (C2rtError, ERR_UNSUPPORTED)."""
        frame = np.empty((opts.height, opts.width, 3), dtype=np.float32)
        mask = np.empty((opts.height, opts.width), dtype=np.uint8)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self._check(self._lib.c2rt_render_frame_adaptive(self._h, C.byref(cam), C.byref(opts), float(threshold),
                                                         frame.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), stop))
        return frame, mask

    def renderFrameAdaptiveDevice(self, cam, opts, out_ptr, mask_ptr, threshold=_abi.AA_THRESHOLD_REF, stream=0):
        """Enqueue the adaptive frame on `stream` into device memory: H * W * 3 floats at out_ptr, H * W bytes at
        mask_ptr (required: it is the buffer between the detection and the refinement kernel)."""
        self._check(self._lib.c2rt_render_frame_adaptive_device(self._h, C.byref(cam), C.byref(opts), float(threshold),
                                                                C.c_void_p(out_ptr or None), C.c_void_p(mask_ptr or None), C.c_void_p(stream)))

    def renderFrameTaps(self, cam, opts, taps):
        """A frame sampled through the caller's tap table (c2rt_render_frame_taps): a new host array of shape
        (local_rows, W, 3), every pixel the sum of its taps' colours in tap order divided by their count.  `taps`: a
        TapTable or a sequence of up to 16 (dx, dy) — TAPS_REF5_TABLE gives the bits of the TAPS_REF5 frame, tap_grid(4)
        a 4x4 grid.  opts.taps is ignored.  No depth of field, stereo, count_rays or prepass_bucket (ERR_UNSUPPORTED)."""
        out = np.empty((self.localRows(opts), opts.width, 3), dtype=np.float32)
        self._check(self._lib.c2rt_render_frame_taps(self._h, C.byref(cam), C.byref(opts), C.byref(_tap_table(taps)), out.ctypes.data_as(C.c_void_p)))
        return out

    def renderFrameTapsDevice(self, cam, opts, taps, out_ptr, stream=0):
        """Enqueue the same frame into device memory (local_rows * W * 3 floats at out_ptr) on `stream`: one kernel."""
        self._check(self._lib.c2rt_render_frame_taps_device(self._h, C.byref(cam), C.byref(opts), C.byref(_tap_table(taps)), C.c_void_p(out_ptr or None),
                                                            C.c_void_p(stream)))

    def renderFrameAdaptiveTaps(self, cam, opts, taps, threshold=_abi.AA_THRESHOLD_REF, stop_flag=None):
        """renderFrameAdaptive with taps 1 .. n-1 of the caller's table on the flagged pixels
        (c2rt_render_frame_adaptive_taps; n >= 2, tap 0 at (0, 0)): (frame, mask).  A flagged pixel holds the bits of
        renderFrameTaps for the same table, an unflagged one the bits of the one-tap frame."""
        frame = np.empty((opts.height, opts.width, 3), dtype=np.float32)
        mask = np.empty((opts.height, opts.width), dtype=np.uint8)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self._check(self._lib.c2rt_render_frame_adaptive_taps(self._h, C.byref(cam), C.byref(opts), C.byref(_tap_table(taps)), float(threshold),
                                                              frame.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), stop))
        return frame, mask

    def renderFrameAdaptiveTapsDevice(self, cam, opts, taps, out_ptr, mask_ptr, threshold=_abi.AA_THRESHOLD_REF, stream=0):
        """Enqueue the same on `stream` into device memory: H * W * 3 floats at out_ptr, H * W bytes at mask_ptr (required)."""
        self._check(self._lib.c2rt_render_frame_adaptive_taps_device(self._h, C.byref(cam), C.byref(opts), C.byref(_tap_table(taps)), float(threshold),
                                                                     C.c_void_p(out_ptr or None), C.c_void_p(mask_ptr or None), C.c_void_p(stream)))

    def renderFramesAdaptive(self, cams, opts, threshold=_abi.AA_THRESHOLD_REF, stop_flag=None):
        """Adaptive anti-aliasing for a batch of cameras (c2rt_render_frames_adaptive; opts.taps must be TAPS_REF5):
        (frames, masks) of shapes (len(cams), H, W, 3) float32 and (len(cams), H, W) uint8; frame i and mask i hold
        the bits renderFrameAdaptive(cams[i], opts, threshold) returns.  One detection and one refinement launch for
        all frames.  What a batch and what an adaptive frame refuse, this refuses (C2rtError)."""
        arr, n = self._camera_array(cams)
        frames = np.empty((n, opts.height, opts.width, 3), dtype=np.float32)
        masks = np.empty((n, opts.height, opts.width), dtype=np.uint8)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self._check(self._lib.c2rt_render_frames_adaptive(self._h, arr, n, C.byref(opts), float(threshold),
                                                          frames.ctypes.data_as(C.c_void_p), masks.ctypes.data_as(C.c_void_p), stop))
        return frames, masks

    def renderFramesAdaptiveDevice(self, cams, opts, out_ptr, mask_ptr, threshold=_abi.AA_THRESHOLD_REF, stream=0):
        """Enqueue the adaptive batch on `stream` into device memory: len(cams) * H * W * 3 floats at out_ptr and
        len(cams) * H * W bytes at mask_ptr (required)."""
        arr, n = self._camera_array(cams)
        self._check(self._lib.c2rt_render_frames_adaptive_device(self._h, arr, n, C.byref(opts), float(threshold),
                                                                 C.c_void_p(out_ptr or None), C.c_void_p(mask_ptr or None), C.c_void_p(stream)))

    def renderFramesPosedAdaptive(self, cams, poses, opts, threshold=_abi.AA_THRESHOLD_REF, stop_flag=None):
        """An anti-aliased animation in one call (c2rt_render_frames_posed_adaptive): renderFramesAdaptive with poses[i]
        — given as renderFramesPosed takes them, each relative to the current scene — applied to frame i.  The
        context's scene is unchanged."""
        arr, parr, n, keep = self._posed_arrays(cams, poses)
        frames = np.empty((n, opts.height, opts.width, 3), dtype=np.float32)
        masks = np.empty((n, opts.height, opts.width), dtype=np.uint8)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self._check(self._lib.c2rt_render_frames_posed_adaptive(self._h, arr, parr, n, C.byref(opts), float(threshold),
                                                                frames.ctypes.data_as(C.c_void_p), masks.ctypes.data_as(C.c_void_p), stop))
        return frames, masks

    def renderFramesPosedAdaptiveDevice(self, cams, poses, opts, out_ptr, mask_ptr, threshold=_abi.AA_THRESHOLD_REF, stream=0):
        """Enqueue the posed adaptive batch on `stream` into device memory, laid out as for renderFramesAdaptiveDevice."""
        arr, parr, n, keep = self._posed_arrays(cams, poses)
        self._check(self._lib.c2rt_render_frames_posed_adaptive_device(self._h, arr, parr, n, C.byref(opts), float(threshold),
                                                                       C.c_void_p(out_ptr or None), C.c_void_p(mask_ptr or None), C.c_void_p(stream)))

    def rayStats(self):
        s = RayStats()
        self._check(self._lib.c2rt_get_ray_stats(self._h, C.byref(s)))
        return int(s.primary_rays), int(s.shadow_rays)

    def csgTruncations(self):
        """CsgOp child hit lists that reached C2RT_MAX_CSG_HITS during the last counted frame."""
        n = C.c_uint64()
        self._check(self._lib.c2rt_get_csg_truncations(self._h, C.byref(n)))
        return int(n.value)

    def exactRedos(self):
        """Tiles this context has rendered a second time through the compiler's divide / sqrt (cumulative)."""
        n = C.c_uint64()
        self._check(self._lib.c2rt_get_exact_redos(self._h, C.byref(n)))
        return int(n.value)

    def groundBails(self):
        """Ground-only tiles that left the short fp64 chain for the full one (cumulative; ground_certain.h)."""
        n = C.c_uint64()
        self._check(self._lib.c2rt_get_ground_bails(self._h, C.byref(n)))
        return int(n.value)

    def sphereBails(self):
        """Sphere-interior tiles handed back to the general path (cumulative; csg_void.h: the proof says 0)."""
        n = C.c_uint64()
        self._check(self._lib.c2rt_get_sphere_bails(self._h, C.byref(n)))
        return int(n.value)

    def csgTileBails(self):
        """Ground-and-CsgOp tiles handed back to the general path (cumulative; c2rt_trace.inc: csg_tile)."""
        n = C.c_uint64()
        self._check(self._lib.c2rt_get_csg_tile_bails(self._h, C.byref(n)))
        return int(n.value)

    def csgTiles(self):
        """Tiles csg_tile rendered (cumulative; counted by the lane-statistics library only, 0 elsewhere)."""
        n = C.c_uint64()
        self._check(self._lib.c2rt_get_csg_tiles(self._h, C.byref(n)))
        return int(n.value)

    def renderPixel(self, cam, opts, x, y):
        r = TraceResult()
        self._check(self._lib.c2rt_render_pixel(self._h, C.byref(cam), C.byref(opts), int(x), int(y), C.byref(r)))
        return r

    def traceRays(self, rays, hits=True, colors=True):
        """Closest hit and colour of caller-supplied rays (c2rt_trace_rays): `rays` is (n, 6) float64 — origin, then the
        direction, used exactly as given.  Returns (records, rgb): a structured array of RAY_HIT_DTYPE (c2rt_ray_hit)
        and an (n, 3) float32 array; the one switched off is None (colors=False casts no shadow ray)."""
        rays = _rays_array(rays)
        n = rays.shape[0]
        rec = np.empty(n, dtype=RAY_HIT_DTYPE) if hits else None
        rgb = np.empty((n, 3), dtype=np.float32) if colors else None
        self._check(self._lib.c2rt_trace_rays(self._h, rays.ctypes.data_as(C.c_void_p), n,
                                              rec.ctypes.data_as(C.c_void_p) if hits else None,
                                              rgb.ctypes.data_as(C.c_void_p) if colors else None))
        return rec, rgb

    def traceRaysDevice(self, rays_ptr, n, hits_ptr, rgb_ptr, stream=0):
        """Enqueue the query on `stream` over device memory: n c2rt_ray at rays_ptr, n c2rt_ray_hit at hits_ptr and
        n * 3 floats at rgb_ptr (either output may be 0 / None, not both)."""
        self._check(self._lib.c2rt_trace_rays_device(self._h, C.c_void_p(rays_ptr), int(n), C.c_void_p(hits_ptr or None),
                                                     C.c_void_p(rgb_ptr or None), C.c_void_p(stream)))

    def traceRayLayers(self, rays, max_layers, hits=True, colors=True):
        """Every surface along caller-supplied rays, in order (c2rt_trace_rays_layers): `rays` as for traceRays.  Returns
        (records, rgb, count): records (max_layers, n) of RAY_HIT_DTYPE and rgb (max_layers, n, 3) float32, layer k of ray
        i at [k, i] — the one switched off is None — and count (n,) uint8, the number of hits stored.  Slot [k, i] means
        something for k <= count[i] only (the miss that ended the walk is stored; what lies behind it is unspecified)."""
        rays = _rays_array(rays)
        n, K = rays.shape[0], int(max_layers)
        rec = np.zeros((max(K, 0), n), dtype=RAY_HIT_DTYPE) if hits else None
        rgb = np.zeros((max(K, 0), n, 3), dtype=np.float32) if colors else None
        count = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.c2rt_trace_rays_layers(self._h, rays.ctypes.data_as(C.c_void_p), n, K,
                                                     rec.ctypes.data_as(C.c_void_p) if hits else None,
                                                     rgb.ctypes.data_as(C.c_void_p) if colors else None,
                                                     count.ctypes.data_as(C.c_void_p)))
        return rec, rgb, count

    def traceRayLayersDevice(self, rays_ptr, n, max_layers, hits_ptr, rgb_ptr, count_ptr, stream=0):
        """Enqueue the layer query on `stream` over device memory: n c2rt_ray at rays_ptr, max_layers * n c2rt_ray_hit at
        hits_ptr, max_layers * n * 3 floats at rgb_ptr (layer-major), n bytes at count_ptr; any output may be 0 / None,
        not all three.  Slots behind a ray's final miss are not touched."""
        self._check(self._lib.c2rt_trace_rays_layers_device(self._h, C.c_void_p(rays_ptr), int(n), int(max_layers), C.c_void_p(hits_ptr or None),
                                                            C.c_void_p(rgb_ptr or None), C.c_void_p(count_ptr or None), C.c_void_p(stream)))

    def renderHitLayers(self, cam, opts, max_layers, planes=("node", "leaf", "dist", "uv", "p", "normal", "rgb")):
        """Every surface behind every pixel of the frame (c2rt_render_hit_layers): a dict of numpy arrays for the planes
        named, shaped (max_layers, local_rows, W) or (max_layers, local_rows, W, components) — layer k is the k-th surface
        along the pixel's ray, layer 0 what renderHits returns — plus "count" (local_rows, W) uint8.  A pixel's layer k
        means something for k <= count only.  Refuses what renderHits refuses."""
        K, rows = int(max_layers), self.localRows(opts)
        pl, out = _HIT.new(planes, (max(K, 0) * rows, opts.width))
        count = np.zeros((rows, opts.width), dtype=np.uint8)
        self._check(self._lib.c2rt_render_hit_layers(self._h, C.byref(cam), C.byref(opts), K, C.byref(pl), count.ctypes.data_as(C.c_void_p)))
        out = {k: v.reshape((K, rows) + v.shape[1:]) for k, v in out.items()}
        out["count"] = count
        return out

    def renderHitLayersDevice(self, cam, opts, max_layers, ptrs, count_ptr=0, stream=0):
        """Enqueue the hit layers on `stream` into device memory: `ptrs` maps plane names (HIT_PLANES) to device pointers
        of max_layers * local_rows * W * components elements, layer after layer without padding; count_ptr: local_rows * W
        bytes.  Planes left out (or 0 / None) are not written; slots behind a pixel's final miss are not touched."""
        pl = _HIT.device(ptrs)
        self._check(self._lib.c2rt_render_hit_layers_device(self._h, C.byref(cam), C.byref(opts), int(max_layers), C.byref(pl),
                                                            C.c_void_p(count_ptr or None), C.c_void_p(stream)))

    def renderHits(self, cam, opts, planes=("node", "leaf", "dist", "uv", "p", "normal", "rgb")):
        """What every pixel of the frame hit (c2rt_render_hits): a dict of numpy arrays for the planes named — node,
        leaf (int32) and dist (float64) of shape (local_rows, W), uv (local_rows, W, 2), p and normal (local_rows, W, 3)
        float64, rgb (local_rows, W, 3) float32: renderPixel(x, y)'s record at [y, x].  Planes not named are neither
        computed nor stored.  No depth of field, stereo, count_rays or prepass_bucket (C2rtError, ERR_UNSUPPORTED)."""
        pl, out = _HIT.new(planes, (self.localRows(opts), opts.width))
        self._check(self._lib.c2rt_render_hits(self._h, C.byref(cam), C.byref(opts), C.byref(pl)))
        return out

    def renderHitsDevice(self, cam, opts, ptrs, stream=0):
        """Enqueue the hit planes on `stream` into device memory: `ptrs` maps plane names (HIT_PLANES) to device
        pointers of local_rows * W * components elements; planes left out (or 0 / None) are not written."""
        pl = _HIT.device(ptrs)
        self._check(self._lib.c2rt_render_hits_device(self._h, C.byref(cam), C.byref(opts), C.byref(pl), C.c_void_p(stream)))

    def renderFramesHits(self, cams, opts, planes=("node", "leaf", "dist", "uv", "p", "normal", "rgb")):
        """The hit planes of a batch of cameras in one call (c2rt_render_frames_hits): a dict of numpy arrays for the
        planes named, shaped (len(cams), local_rows, W) or (len(cams), local_rows, W, components); slice i holds the
        bits renderHits(cams[i], opts, planes) returns.  What a batch refuses, this refuses (C2rtError)."""
        arr, n = self._camera_array(cams)
        rows = self.localRows(opts)
        pl, out = _HIT.new(planes, (n * rows, opts.width))
        self._check(self._lib.c2rt_render_frames_hits(self._h, arr, n, C.byref(opts), C.byref(pl)))
        return {k: v.reshape((n, rows) + v.shape[1:]) for k, v in out.items()}

    def renderFramesHitsDevice(self, cams, opts, ptrs, stream=0):
        """Enqueue the batch's hit planes on `stream` into device memory, one launch for all frames: `ptrs` maps plane
        names (HIT_PLANES) to device pointers of len(cams) * local_rows * W * components elements, frame after frame
        without padding; planes left out (or 0 / None) are not written."""
        arr, n = self._camera_array(cams)
        pl = _HIT.device(ptrs)
        self._check(self._lib.c2rt_render_frames_hits_device(self._h, arr, n, C.byref(opts), C.byref(pl), C.c_void_p(stream)))

    def renderFramesPosedHits(self, cams, poses, opts, planes=("node", "leaf", "dist", "uv", "p", "normal", "rgb")):
        """The hit planes of a posed animation in one call (c2rt_render_frames_posed_hits): renderFramesHits with
        poses[i] — given as renderFramesPosed takes them, each relative to the current scene — applied to frame i: the
        bits of updateScene(poses[i]) + renderHits(cams[i]).  The context's scene is unchanged."""
        arr, parr, n, keep = self._posed_arrays(cams, poses)
        rows = self.localRows(opts)
        pl, out = _HIT.new(planes, (n * rows, opts.width))
        self._check(self._lib.c2rt_render_frames_posed_hits(self._h, arr, parr, n, C.byref(opts), C.byref(pl)))
        return {k: v.reshape((n, rows) + v.shape[1:]) for k, v in out.items()}

    def renderFramesPosedHitsDevice(self, cams, poses, opts, ptrs, stream=0):
        """Enqueue the posed batch's hit planes on `stream` into device memory, laid out as for renderFramesHitsDevice."""
        arr, parr, n, keep = self._posed_arrays(cams, poses)
        pl = _HIT.device(ptrs)
        self._check(self._lib.c2rt_render_frames_posed_hits_device(self._h, arr, parr, n, C.byref(opts), C.byref(pl), C.c_void_p(stream)))

    def renderShading(self, cam, opts, planes=tuple(SHADE_PLANES)):
        """The terms of every pixel's colour (c2rt_render_shading): a dict of numpy arrays for the planes named — node
        (int32) and visible (uint32, bit l: light l < 32 passed the shadow test) of shape (local_rows, W); albedo, light,
        specular and rgb (local_rows, W, 3) float32.  On a hit rgb == albedo * light (+ specular for a Phong node) bit for
        bit, and rgb and node are renderHits'.  Planes not named are neither computed nor stored; node and albedo alone
        cast no shadow ray.  Refuses what renderHits refuses."""
        pl, out = _SHADE.new(planes, (self.localRows(opts), opts.width))
        self._check(self._lib.c2rt_render_shading(self._h, C.byref(cam), C.byref(opts), C.byref(pl)))
        return out

    def renderShadingDevice(self, cam, opts, ptrs, stream=0):
        """Enqueue the shading planes on `stream` into device memory: `ptrs` maps plane names (SHADE_PLANES) to device
        pointers of local_rows * W * components elements; planes left out (or 0 / None) are not written."""
        pl = _SHADE.device(ptrs)
        self._check(self._lib.c2rt_render_shading_device(self._h, C.byref(cam), C.byref(opts), C.byref(pl), C.c_void_p(stream)))

    def traceRaysShading(self, rays, planes=tuple(SHADE_PLANES)):
        """The same terms for caller-supplied rays (c2rt_trace_rays_shading): `rays` as for traceRays; a dict of arrays of
        shape (n,) or (n, 3).  rgb and node are traceRays'."""
        rays = _rays_array(rays)
        pl, out = _SHADE.new(planes, (rays.shape[0],))
        self._check(self._lib.c2rt_trace_rays_shading(self._h, rays.ctypes.data_as(C.c_void_p), rays.shape[0], C.byref(pl)))
        return out

    def traceRaysShadingDevice(self, rays_ptr, n, ptrs, stream=0):
        """Enqueue the query on `stream` over device memory: n c2rt_ray at rays_ptr, `ptrs` as for renderShadingDevice
        with n samples per plane."""
        pl = _SHADE.device(ptrs)
        self._check(self._lib.c2rt_trace_rays_shading_device(self._h, C.c_void_p(rays_ptr or None), int(n), C.byref(pl), C.c_void_p(stream)))

    def renderOcclusion(self, cam, opts, samples, radius, seed=0, planes=tuple(OCCLUSION_PLANES)):
        """Ambient occlusion of every pixel's closest hit (c2rt_render_occlusion): `samples` (1 .. 64) segments of length
        `radius` over the hemisphere around the hit's normal, each answered by the library's visibility test.  A dict of
        numpy arrays for the planes named — node (int32), open (uint64, bit s: sample s is unoccluded) and ao (float32,
        the open fraction) of shape (local_rows, W); bent (local_rows, W, 3) float64, the sum of the open directions.  A
        miss holds -1, the low `samples` bits, 1.0 and zeros.  node alone traces no sample.  Refuses what renderHits
        refuses."""
        occ = _occlusion_opts(samples, radius, seed)
        pl, out = _OCCLUSION.new(planes, (self.localRows(opts), opts.width))
        self._check(self._lib.c2rt_render_occlusion(self._h, C.byref(cam), C.byref(opts), C.byref(occ), C.byref(pl)))
        return out

    def renderOcclusionDevice(self, cam, opts, samples, radius, ptrs, seed=0, stream=0):
        """Enqueue the occlusion planes on `stream` into device memory: `ptrs` maps plane names (OCCLUSION_PLANES) to
        device pointers of local_rows * W * components elements; planes left out (or 0 / None) are not written."""
        occ = _occlusion_opts(samples, radius, seed)
        pl = _OCCLUSION.device(ptrs)
        self._check(self._lib.c2rt_render_occlusion_device(self._h, C.byref(cam), C.byref(opts), C.byref(occ), C.byref(pl), C.c_void_p(stream)))

    def traceRaysOcclusion(self, rays, samples, radius, seed=0, planes=tuple(OCCLUSION_PLANES)):
        """The same planes for caller-supplied rays (c2rt_trace_rays_occlusion): `rays` as for traceRays; a dict of arrays
        of shape (n,) or (n, 3).  Ray i draws the samples of index i; node is traceRays'."""
        rays = _rays_array(rays)
        occ = _occlusion_opts(samples, radius, seed)
        pl, out = _OCCLUSION.new(planes, (rays.shape[0],))
        self._check(self._lib.c2rt_trace_rays_occlusion(self._h, rays.ctypes.data_as(C.c_void_p), rays.shape[0], C.byref(occ), C.byref(pl)))
        return out

    def traceRaysOcclusionDevice(self, rays_ptr, n, samples, radius, ptrs, seed=0, stream=0):
        """Enqueue the query on `stream` over device memory: n c2rt_ray at rays_ptr, `ptrs` as for renderOcclusionDevice
        with n samples per plane."""
        occ = _occlusion_opts(samples, radius, seed)
        pl = _OCCLUSION.device(ptrs)
        self._check(self._lib.c2rt_trace_rays_occlusion_device(self._h, C.c_void_p(rays_ptr or None), int(n), C.byref(occ), C.byref(pl),
                                                               C.c_void_p(stream)))

    def renderGather(self, cam, opts, samples, seed=0, planes=tuple(GATHER_PLANES)):
        """One-bounce indirect diffuse light of every pixel's closest hit (c2rt_render_gather): `samples` (1 .. 64) rays
        over the hemisphere around the hit's normal, each traced and shaded as traceRays does.  A dict of numpy arrays
        for the planes named — node (int32) and hits (uint64, bit s: sample s's ray hit a node) of shape (local_rows,
        W); indirect and bounce (local_rows, W, 3) float32: the mean weighted colour arriving, and that times the hit's
        albedo — what to add to the frame's colour.  A miss holds -1, 0 and zeros.  node alone traces no sample.
        Refuses what renderHits refuses."""
        g = _gather_opts(samples, seed)
        pl, out = _GATHER.new(planes, (self.localRows(opts), opts.width))
        self._check(self._lib.c2rt_render_gather(self._h, C.byref(cam), C.byref(opts), C.byref(g), C.byref(pl)))
        return out

    def renderGatherDevice(self, cam, opts, samples, ptrs, seed=0, stream=0):
        """Enqueue the gather planes on `stream` into device memory: `ptrs` maps plane names (GATHER_PLANES) to device
        pointers of local_rows * W * components elements; planes left out (or 0 / None) are not written."""
        g = _gather_opts(samples, seed)
        pl = _GATHER.device(ptrs)
        self._check(self._lib.c2rt_render_gather_device(self._h, C.byref(cam), C.byref(opts), C.byref(g), C.byref(pl), C.c_void_p(stream)))

    def traceRaysGather(self, rays, samples, seed=0, planes=tuple(GATHER_PLANES)):
        """The same planes for caller-supplied rays (c2rt_trace_rays_gather): `rays` as for traceRays; a dict of arrays of
        shape (n,) or (n, 3).  Ray i draws the samples of index i; node is traceRays'."""
        rays = _rays_array(rays)
        g = _gather_opts(samples, seed)
        pl, out = _GATHER.new(planes, (rays.shape[0],))
        self._check(self._lib.c2rt_trace_rays_gather(self._h, rays.ctypes.data_as(C.c_void_p), rays.shape[0], C.byref(g), C.byref(pl)))
        return out

    def traceRaysGatherDevice(self, rays_ptr, n, samples, ptrs, seed=0, stream=0):
        """Enqueue the query on `stream` over device memory: n c2rt_ray at rays_ptr, `ptrs` as for renderGatherDevice with
        n samples per plane."""
        g = _gather_opts(samples, seed)
        pl = _GATHER.device(ptrs)
        self._check(self._lib.c2rt_trace_rays_gather_device(self._h, C.c_void_p(rays_ptr or None), int(n), C.byref(g), C.byref(pl), C.c_void_p(stream)))

    def renderPaths(self, cam, opts, paths, bounces, seed=0, planes=tuple(PATH_PLANES)):
        """Multi-bounce indirect diffuse light of every pixel's closest hit (c2rt_render_paths): `paths` (1 .. 64) paths
        of at most min(`bounces` (1 .. 8), the scene's max_trace_depth) segments behind the hit, every segment shaded as
        traceRays shades a ray.  Planes (PATH_PLANES): node, segments (how many spawned segments hit a node), indirect,
        bounce (albedo * indirect), radiance (the frame's colour + bounce); a dict of arrays of shape (localRows, width)
        and (localRows, width, 3).  With bounces == 1: renderGather's indirect and bounce at samples == paths.  Depth of
        field, stereo, count_rays and prepass_bucket are refused."""
        g = _path_opts(paths, bounces, seed)
        pl, out = _PATHS.new(planes, (self.localRows(opts), opts.width))
        self._check(self._lib.c2rt_render_paths(self._h, C.byref(cam), C.byref(opts), C.byref(g), C.byref(pl)))
        return out

    def renderPathsDevice(self, cam, opts, paths, bounces, ptrs, seed=0, stream=0):
        """Enqueue the path planes on `stream` into device memory: `ptrs` maps plane names (PATH_PLANES) to device
        pointers; planes left out are not computed."""
        g = _path_opts(paths, bounces, seed)
        pl = _PATHS.device(ptrs)
        self._check(self._lib.c2rt_render_paths_device(self._h, C.byref(cam), C.byref(opts), C.byref(g), C.byref(pl), C.c_void_p(stream)))

    def traceRaysPaths(self, rays, paths, bounces, seed=0, planes=tuple(PATH_PLANES)):
        """The same planes for caller-supplied rays (c2rt_trace_rays_paths): `rays` as for traceRays; a dict of arrays of
        shape (n,) and (n, 3).  Ray i draws the paths of index i."""
        rays = _rays_array(rays)
        g = _path_opts(paths, bounces, seed)
        pl, out = _PATHS.new(planes, (rays.shape[0],))
        self._check(self._lib.c2rt_trace_rays_paths(self._h, rays.ctypes.data_as(C.c_void_p), rays.shape[0], C.byref(g), C.byref(pl)))
        return out

    def traceRaysPathsDevice(self, rays_ptr, n, paths, bounces, ptrs, seed=0, stream=0):
        """Enqueue the query on `stream` over device memory: n c2rt_ray at rays_ptr, `ptrs` as for renderPathsDevice with
        n samples per plane."""
        g = _path_opts(paths, bounces, seed)
        pl = _PATHS.device(ptrs)
        self._check(self._lib.c2rt_trace_rays_paths_device(self._h, C.c_void_p(rays_ptr or None), int(n), C.byref(g), C.byref(pl), C.c_void_p(stream)))

    def renderPathsCounted(self, cam, opts, counts, paths, bounces, seed=0, planes=tuple(PATH_PLANES)):
        """renderPaths with a path count per pixel (c2rt_render_paths_counted): `counts` (localRows, width) uint8; pixel i
        is traced with c = min(counts[i], paths) paths and holds, bit for bit, what renderPaths writes for it with
        paths = c; c == 0: node and the primary colour only, indirect = bounce = 0."""
        g = _path_opts(paths, bounces, seed)
        shape = (self.localRows(opts), opts.width)
        counts = _counts_array(counts, shape, "renderPathsCounted")
        pl, out = _PATHS.new(planes, shape)
        self._check(self._lib.c2rt_render_paths_counted(self._h, C.byref(cam), C.byref(opts), C.byref(g), counts.ctypes.data_as(C.c_void_p), C.byref(pl)))
        return out

    def renderPathsCountedDevice(self, cam, opts, counts_ptr, paths, bounces, ptrs, seed=0, scratch_ptr=0, stream=0):
        """Enqueue the counted path planes on `stream` into device memory: `counts_ptr` one byte per pixel, `ptrs` as for
        renderPathsDevice.  scratch_ptr 0: natural order, one kernel; else paths_counted_scratch_bytes(localRows * width)
        bytes, 16-byte aligned: count order (a counting sort of the pixels by their count ahead of the path kernel) —
        the same bits."""
        g = _path_opts(paths, bounces, seed)
        pl = _PATHS.device(ptrs)
        self._check(self._lib.c2rt_render_paths_counted_device(self._h, C.byref(cam), C.byref(opts), C.byref(g), C.c_void_p(counts_ptr or None), C.byref(pl),
                                                               C.c_void_p(scratch_ptr or None), C.c_void_p(stream)))

    def traceRaysPathsCounted(self, rays, counts, paths, bounces, seed=0, planes=tuple(PATH_PLANES)):
        """traceRaysPaths with a path count per ray (c2rt_trace_rays_paths_counted): `counts` (n,) uint8."""
        rays = _rays_array(rays)
        g = _path_opts(paths, bounces, seed)
        counts = _counts_array(counts, (rays.shape[0],), "traceRaysPathsCounted")
        pl, out = _PATHS.new(planes, (rays.shape[0],))
        self._check(self._lib.c2rt_trace_rays_paths_counted(self._h, rays.ctypes.data_as(C.c_void_p), rays.shape[0], C.byref(g),
                                                            counts.ctypes.data_as(C.c_void_p), C.byref(pl)))
        return out

    def traceRaysPathsCountedDevice(self, rays_ptr, n, counts_ptr, paths, bounces, ptrs, seed=0, scratch_ptr=0, stream=0):
        """Enqueue the counted query on `stream` over device memory: n c2rt_ray at rays_ptr, n bytes at counts_ptr, `ptrs`
        and scratch_ptr (for n samples) as for renderPathsCountedDevice."""
        g = _path_opts(paths, bounces, seed)
        pl = _PATHS.device(ptrs)
        self._check(self._lib.c2rt_trace_rays_paths_counted_device(self._h, C.c_void_p(rays_ptr or None), int(n), C.byref(g), C.c_void_p(counts_ptr or None),
                                                                   C.byref(pl), C.c_void_p(scratch_ptr or None), C.c_void_p(stream)))

    def pathCounts(self, guides, prev_cam=None, history=None, prev_counts=None, min_paths=PATH_COUNT_MIN, max_paths=PATH_COUNT_MAX,
                   young_paths=PATH_COUNT_YOUNG, min_age=PATH_COUNT_MIN_AGE, paths_per_variance=PATH_COUNT_PER_VARIANCE, prev_paths=PATH_COUNT_YOUNG,
                   channels=3, min_normal_dot=TEMPORAL_MIN_NORMAL_DOT, max_plane_dist=TEMPORAL_MAX_PLANE_DIST, planes=("variance", "age")):
        """The counts plane of renderPathsCounted for the frame whose hit planes are `guides`, from the PREVIOUS history
        (c2rt_path_counts): every pixel's point is projected into `prev_cam` and the history's luminance moments, age and
        — from `prev_counts` (H, W) uint8, or `prev_paths` everywhere — the count its last sample was traced with are
        gathered as temporalAccumulate gathers them; counts = ceil(variance * previous count * paths_per_variance) within
        min_paths .. max_paths, `young_paths` without a history or below `min_age`, 0 at a miss.  `channels`: the
        history's.  Returns {"counts": (H, W) uint8, and of `planes`: "variance" float32, "age" uint32}."""
        keep = [np.ascontiguousarray(guides["node"], dtype=np.int32), np.ascontiguousarray(guides["normal"], dtype=np.float64),
                np.ascontiguousarray(guides["p"], dtype=np.float64)]
        if keep[0].ndim != 2:
            raise ValueError("pathCounts: guide node of shape %r (expected (H, W))" % (keep[0].shape,))
        h, w = keep[0].shape
        for a, shape, name in zip(keep, ((h, w), (h, w, 3), (h, w, 3)), ("node", "normal", "p")):
            if a.shape != shape:
                raise ValueError("pathCounts: guide %s of shape %r (expected %r)" % (name, a.shape, shape))
        g = TemporalGuides(node=keep[0].ctypes.data, normal=keep[1].ctypes.data, p=keep[2].ctypes.data)
        o = _temporal_opts(w, h, channels, 1, min_normal_dot, max_plane_dist)
        pc = _path_count_opts(min_paths, max_paths, young_paths, min_age, paths_per_variance, prev_paths)
        prev = None
        if history is not None:
            prev = np.ascontiguousarray(np.frombuffer(history, dtype=np.uint8))
            if prev.size != w * h * (32 + 4 * channels + 8):
                raise ValueError("pathCounts: history of %d bytes (expected %d)" % (prev.size, w * h * (32 + 4 * channels + 8)))
        pcn = None if prev_counts is None else _counts_array(prev_counts, (h, w), "pathCounts")
        out = {"counts": np.empty((h, w), dtype=np.uint8)}
        for n in planes:
            if n not in ("variance", "age"):
                raise ValueError("unknown path count plane %r (one of variance, age)" % (n,))
            out[n] = np.empty((h, w), dtype=TEMPORAL_PLANES[n])
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.c2rt_path_counts(self._h, None if prev_cam is None else C.byref(prev_cam), C.byref(g), C.byref(o), C.byref(pc), ptr(prev),
                                               ptr(pcn), ptr(out["counts"]), ptr(out.get("variance")), ptr(out.get("age"))))
        return out

    def pathCountsDevice(self, ptrs, width, height, history_prev_ptr, prev_counts_ptr, counts_ptr, variance_ptr=0, age_ptr=0, prev_cam=None,
                         min_paths=PATH_COUNT_MIN, max_paths=PATH_COUNT_MAX, young_paths=PATH_COUNT_YOUNG, min_age=PATH_COUNT_MIN_AGE,
                         paths_per_variance=PATH_COUNT_PER_VARIANCE, prev_paths=PATH_COUNT_YOUNG, channels=3, min_normal_dot=TEMPORAL_MIN_NORMAL_DOT,
                         max_plane_dist=TEMPORAL_MAX_PLANE_DIST, stream=0):
        """Enqueue the count rule on `stream` over device memory (c2rt_path_counts_device): `ptrs` maps node, normal and p
        to the current frame's planes; history_prev_ptr (16-byte aligned; 0: the first frame) and prev_counts_ptr (0:
        prev_paths everywhere) the previous frame's; width * height bytes at counts_ptr; variance_ptr and age_ptr 0 or
        float32 / uint32 planes.  One kernel, no sync."""
        g = TemporalGuides()
        for n, ptr in dict(ptrs).items():
            if n not in ("node", "normal", "p"):
                raise ValueError("unknown temporal guide %r (one of node, normal, p)" % (n,))
            setattr(g, n, ptr or None)
        o = _temporal_opts(width, height, channels, 1, min_normal_dot, max_plane_dist)
        pc = _path_count_opts(min_paths, max_paths, young_paths, min_age, paths_per_variance, prev_paths)
        self._check(self._lib.c2rt_path_counts_device(self._h, None if prev_cam is None else C.byref(prev_cam), C.byref(g), C.byref(o), C.byref(pc),
                                                      C.c_void_p(history_prev_ptr or None), C.c_void_p(prev_counts_ptr or None), C.c_void_p(counts_ptr or None),
                                                      C.c_void_p(variance_ptr or None), C.c_void_p(age_ptr or None), C.c_void_p(stream)))

    def denoise(self, guides, image, levels=5, normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE, sigma_colour=0.0, albedo=None, base=None):
        """Edge-aware a-trous filter of a Monte-Carlo plane (c2rt_denoise).  `guides`: a dict with the hit planes' node
        (H, W), normal and p (H, W, 3), e.g. what renderHits returns for the WHOLE frame; `image`: (H, W, 3) float32, or
        (H, W) / (H, W, 1) for one channel (renderOcclusion's ao).  `levels` (0 .. 8) 5x5 passes with taps 2^l pixels
        apart; a tap counts only on the centre's node, by dot(n, n')^(2^normal_power_log2), by its distance from the
        centre's tangent plane against `sigma_plane` and, with sigma_colour > 0, by its colour difference.  Then, for
        every pixel, `albedo` (nullable) is multiplied in and `base` (nullable) added: with renderPaths' indirect,
        renderShading's albedo and renderHits' rgb the result is the denoised global-illumination frame.  Returns an
        array of `image`'s shape."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim not in (2, 3):
            raise ValueError("denoise: image of shape %r (expected (H, W), (H, W, 1) or (H, W, 3))" % (image.shape,))
        h, w = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        keep = [np.ascontiguousarray(guides["node"], dtype=np.int32), np.ascontiguousarray(guides["normal"], dtype=np.float64),
                np.ascontiguousarray(guides["p"], dtype=np.float64)]
        for a, shape, name in zip(keep, ((h, w), (h, w, 3), (h, w, 3)), ("node", "normal", "p")):
            if a.shape != shape:
                raise ValueError("denoise: guide %s of shape %r (expected %r)" % (name, a.shape, shape))
        g = DenoiseGuides(node=keep[0].ctypes.data, normal=keep[1].ctypes.data, p=keep[2].ctypes.data)
        for name, a in (("albedo", albedo), ("base", base)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.size != image.size:
                    raise ValueError("denoise: %s of shape %r (expected %r)" % (name, a.shape, image.shape))
                keep.append(a)
                setattr(g, name, a.ctypes.data)
        o = _denoise_opts(w, h, ch, levels, normal_power_log2, sigma_plane, sigma_colour)
        out = np.empty_like(image)
        self._check(self._lib.c2rt_denoise(self._h, C.byref(g), C.byref(o), image.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def denoiseDevice(self, ptrs, width, height, in_ptr, out_ptr, scratch_ptr, channels=3, levels=5, normal_power_log2=5,
                      sigma_plane=DENOISE_SIGMA_PLANE, sigma_colour=0.0, stream=0):
        """Enqueue the filter on `stream` over device memory (c2rt_denoise_device): `ptrs` maps node, normal, p and
        optionally albedo, base to device pointers of full-frame planes; `scratch_ptr`: denoise_scratch_bytes(...) bytes,
        16-byte aligned (0 where that is 0).  No sync; writes only out_ptr and scratch_ptr."""
        g = DenoiseGuides()
        for n, ptr in dict(ptrs).items():
            if n not in ("node", "normal", "p", "albedo", "base"):
                raise ValueError("unknown denoise guide %r (one of node, normal, p, albedo, base)" % (n,))
            setattr(g, n, ptr or None)
        o = _denoise_opts(width, height, channels, levels, normal_power_log2, sigma_plane, sigma_colour)
        self._check(self._lib.c2rt_denoise_device(self._h, C.byref(g), C.byref(o), C.c_void_p(in_ptr or None), C.c_void_p(out_ptr or None),
                                                  C.c_void_p(scratch_ptr or None), C.c_void_p(stream)))

    def renderPathsDenoised(self, cam, opts, paths, bounces, seed=0, levels=5, normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE, sigma_colour=0.0):
        """The global-illumination frame in one call, denoised (c2rt_render_paths_denoised): renderHits' node, normal, p
        and rgb, renderShading's albedo, renderPaths' indirect and denoise(..., albedo=albedo, base=rgb), chained on the
        device; (height, width, 3) float32, bit for bit that composition.  Strips (strip_world > 1) are refused."""
        g = _path_opts(paths, bounces, seed)
        d = _denoise_opts(opts.width, opts.height, 3, levels, normal_power_log2, sigma_plane, sigma_colour)
        out = np.empty((opts.height, opts.width, 3), dtype=np.float32)
        self._check(self._lib.c2rt_render_paths_denoised(self._h, C.byref(cam), C.byref(opts), C.byref(g), C.byref(d), out.ctypes.data_as(C.c_void_p)))
        return out

    def temporalAccumulate(self, guides, image, prev_cam=None, history=None, max_age=TEMPORAL_MAX_AGE, min_normal_dot=TEMPORAL_MIN_NORMAL_DOT,
                           max_plane_dist=TEMPORAL_MAX_PLANE_DIST, planes=("colour", "variance", "age"), motion=None):
        """Temporal accumulation of a Monte-Carlo plane (c2rt_temporal_accumulate; with `motion`,
        c2rt_temporal_accumulate_motion: ``{node index: (prev, cur)}``, see makeMotion — the pixels of those nodes are
        carried from the current pose back into the history's before they are reprojected, so that a moved node finds
        its history; an empty dict is the plain call's bits).  `guides`: a dict with the CURRENT
        frame's node (H, W), normal and p (H, W, 3), e.g. what renderHits returns for the whole frame; `image`: (H, W, 3)
        float32, or (H, W) / (H, W, 1) for one channel.  `history`: the bytes-like history the previous call returned and
        `prev_cam` that call's camera; both None for the first frame.  Every pixel's point is projected into `prev_cam`,
        the history is fetched there from the taps on the same node, within `min_normal_dot` of its normal and
        `max_plane_dist` of its tangent plane, and `image` is folded into a running mean of at most `max_age` samples.
        Returns ({plane: array} for the `planes` asked for — colour of `image`'s shape, variance float32 and age uint32
        (H, W) — and the new history, a uint8 array of temporal_history_bytes(...))."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim not in (2, 3):
            raise ValueError("temporalAccumulate: image of shape %r (expected (H, W), (H, W, 1) or (H, W, 3))" % (image.shape,))
        h, w = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        keep = [np.ascontiguousarray(guides["node"], dtype=np.int32), np.ascontiguousarray(guides["normal"], dtype=np.float64),
                np.ascontiguousarray(guides["p"], dtype=np.float64)]
        for a, shape, name in zip(keep, ((h, w), (h, w, 3), (h, w, 3)), ("node", "normal", "p")):
            if a.shape != shape:
                raise ValueError("temporalAccumulate: guide %s of shape %r (expected %r)" % (name, a.shape, shape))
        g = TemporalGuides(node=keep[0].ctypes.data, normal=keep[1].ctypes.data, p=keep[2].ctypes.data)
        o = _temporal_opts(w, h, ch, max_age, min_normal_dot, max_plane_dist)
        nbytes = w * h * (32 + 4 * ch + 8)
        prev = None
        if history is not None:
            prev = np.ascontiguousarray(np.frombuffer(history, dtype=np.uint8))
            if prev.size != nbytes:
                raise ValueError("temporalAccumulate: history of %d bytes (expected %d)" % (prev.size, nbytes))
        out, pl = {}, TemporalPlanes()
        for n in planes:
            if n not in TEMPORAL_PLANES:
                raise ValueError("unknown temporal plane %r (one of %s)" % (n, ", ".join(TEMPORAL_PLANES)))
            out[n] = np.empty(image.shape if n == "colour" else (h, w), dtype=TEMPORAL_PLANES[n])
            setattr(pl, n, out[n].ctypes.data)
        new = np.empty(nbytes, dtype=np.uint8)
        cam = None if prev_cam is None else C.byref(prev_cam)
        prev_p = None if prev is None else prev.ctypes.data_as(C.c_void_p)
        if motion is None:
            self._check(self._lib.c2rt_temporal_accumulate(self._h, cam, C.byref(g), C.byref(o), image.ctypes.data_as(C.c_void_p), prev_p,
                                                           new.ctypes.data_as(C.c_void_p), C.byref(pl)))
        else:
            m = makeMotion(motion)
            self._check(self._lib.c2rt_temporal_accumulate_motion(self._h, cam, C.byref(g), C.byref(o), C.byref(m), image.ctypes.data_as(C.c_void_p), prev_p,
                                                                  new.ctypes.data_as(C.c_void_p), C.byref(pl)))
        return out, new

    def temporalAccumulateDevice(self, ptrs, width, height, in_ptr, history_prev_ptr, history_out_ptr, planes=None, prev_cam=None, channels=3,
                                 max_age=TEMPORAL_MAX_AGE, min_normal_dot=TEMPORAL_MIN_NORMAL_DOT, max_plane_dist=TEMPORAL_MAX_PLANE_DIST, stream=0,
                                 motion=None):
        """Enqueue the accumulation on `stream` over device memory (c2rt_temporal_accumulate_device; with `motion`, as for
        temporalAccumulate, c2rt_temporal_accumulate_motion_device — the motion is host memory, read before the call returns): `ptrs` maps node,
        normal and p to device pointers of the current frame's planes, `planes` colour, variance and age to the outputs
        wanted (None: the history alone); the histories are temporal_history_bytes(...) bytes each, 16-byte aligned,
        history_prev_ptr 0 for the first frame.  One kernel, no sync; writes only history_out_ptr and `planes`."""
        g = TemporalGuides()
        for n, ptr in dict(ptrs).items():
            if n not in ("node", "normal", "p"):
                raise ValueError("unknown temporal guide %r (one of node, normal, p)" % (n,))
            setattr(g, n, ptr or None)
        pl = TemporalPlanes()
        for n, ptr in dict(planes or {}).items():
            if n not in TEMPORAL_PLANES:
                raise ValueError("unknown temporal plane %r (one of %s)" % (n, ", ".join(TEMPORAL_PLANES)))
            setattr(pl, n, ptr or None)
        o = _temporal_opts(width, height, channels, max_age, min_normal_dot, max_plane_dist)
        cam = None if prev_cam is None else C.byref(prev_cam)
        if motion is None:
            self._check(self._lib.c2rt_temporal_accumulate_device(self._h, cam, C.byref(g), C.byref(o), C.c_void_p(in_ptr or None),
                                                                  C.c_void_p(history_prev_ptr or None), C.c_void_p(history_out_ptr or None), C.byref(pl),
                                                                  C.c_void_p(stream)))
        else:
            m = makeMotion(motion)
            self._check(self._lib.c2rt_temporal_accumulate_motion_device(self._h, cam, C.byref(g), C.byref(o), C.byref(m), C.c_void_p(in_ptr or None),
                                                                         C.c_void_p(history_prev_ptr or None), C.c_void_p(history_out_ptr or None),
                                                                         C.byref(pl), C.c_void_p(stream)))

    def renderPathsSequence(self, cams, opts, paths, bounces, seed=0, max_age=TEMPORAL_MAX_AGE, min_normal_dot=TEMPORAL_MIN_NORMAL_DOT,
                            max_plane_dist=TEMPORAL_MAX_PLANE_DIST, levels=5, normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE, sigma_colour=0.0):
        """A global-illumination sequence in one call (c2rt_render_paths_sequence): for each camera of `cams` renderHits'
        node, normal, p and rgb, renderShading's albedo, renderPaths' indirect with seed + i, temporalAccumulate against
        the previous camera and history, and denoise(..., albedo=albedo, base=rgb), chained on the device; (n, height,
        width, 3) float32, bit for bit that composition."""
        cams = list(cams)
        arr = (CameraFrame * max(len(cams), 1))(*cams)
        g = _path_opts(paths, bounces, seed)
        t = _temporal_opts(opts.width, opts.height, 3, max_age, min_normal_dot, max_plane_dist)
        d = _denoise_opts(opts.width, opts.height, 3, levels, normal_power_log2, sigma_plane, sigma_colour)
        out = np.empty((len(cams), opts.height, opts.width, 3), dtype=np.float32)
        self._check(self._lib.c2rt_render_paths_sequence(self._h, arr, len(cams), C.byref(opts), C.byref(g), C.byref(t), C.byref(d),
                                                         out.ctypes.data_as(C.c_void_p)))
        return out

    def renderPathsSequencePosed(self, cams, poses, opts, paths, bounces, seed=0, max_age=TEMPORAL_MAX_AGE, min_normal_dot=TEMPORAL_MIN_NORMAL_DOT,
                                 max_plane_dist=TEMPORAL_MAX_PLANE_DIST, levels=5, normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE, sigma_colour=0.0):
        """renderPathsSequence for a posed animation (c2rt_render_paths_sequence_posed): frame i is the current scene with
        poses[i] applied — a ScenePose or a (nodes, lights) pair as for renderFramesPosed, each relative to the current
        scene — seen through cams[i]; the accumulation follows the nodes that moved between two frames
        (temporalAccumulate's `motion`).  The context's scene is unchanged.  (n, height, width, 3) float32, bit for bit
        updateScene(poses[i]) + renderHits + renderShading + renderPaths + temporalAccumulate(motion=) + denoise."""
        arr, parr, n, keep = self._posed_arrays(cams, poses)
        g = _path_opts(paths, bounces, seed)
        t = _temporal_opts(opts.width, opts.height, 3, max_age, min_normal_dot, max_plane_dist)
        d = _denoise_opts(opts.width, opts.height, 3, levels, normal_power_log2, sigma_plane, sigma_colour)
        out = np.empty((n, opts.height, opts.width, 3), dtype=np.float32)
        self._check(self._lib.c2rt_render_paths_sequence_posed(self._h, arr, parr, n, C.byref(opts), C.byref(g), C.byref(t), C.byref(d),
                                                               out.ctypes.data_as(C.c_void_p)))
        return out

    def renderPathsSequencePosedVariance(self, cams, poses, opts, paths, bounces, seed=0, max_age=TEMPORAL_MAX_AGE, min_normal_dot=TEMPORAL_MIN_NORMAL_DOT,
                                         max_plane_dist=TEMPORAL_MAX_PLANE_DIST, levels=5, normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE,
                                         sigma_lum=DENOISE_SIGMA_LUM, var_floor=DENOISE_VAR_FLOOR, min_age=DENOISE_MIN_AGE):
        """renderPathsSequencePosed with renderPathsSequenceVariance's filter (c2rt_render_paths_sequence_posed_variance)."""
        arr, parr, n, keep = self._posed_arrays(cams, poses)
        g = _path_opts(paths, bounces, seed)
        t = _temporal_opts(opts.width, opts.height, 3, max_age, min_normal_dot, max_plane_dist)
        d = _denoise_variance_opts(opts.width, opts.height, 3, levels, normal_power_log2, sigma_plane, sigma_lum, var_floor, min_age)
        out = np.empty((n, opts.height, opts.width, 3), dtype=np.float32)
        self._check(self._lib.c2rt_render_paths_sequence_posed_variance(self._h, arr, parr, n, C.byref(opts), C.byref(g), C.byref(t), C.byref(d),
                                                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def denoiseVariance(self, guides, image, variance, age=None, levels=5, normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE,
                        sigma_lum=DENOISE_SIGMA_LUM, var_floor=DENOISE_VAR_FLOOR, min_age=DENOISE_MIN_AGE, albedo=None, base=None, variance_out=True):
        """The a-trous filter steered by the temporal planes (c2rt_denoise_variance).  `guides`, `image`, `albedo` and
        `base` as for denoise; `variance` (H, W) float32 and `age` (H, W) uint32 or None: temporalAccumulate's planes.  In
        place of a colour scale a tap is weighed by its luminance difference in units of `sigma_lum` local standard
        deviations (the 3x3-smoothed variance, plus `var_floor`); the variance is filtered along, and a pixel younger than
        `min_age` gets a variance estimated from its 7x7 neighbourhood.  Returns (out, variance_out): an array of
        `image`'s shape and the (H, W) variance after the last level (None with variance_out=False)."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim not in (2, 3):
            raise ValueError("denoiseVariance: image of shape %r (expected (H, W), (H, W, 1) or (H, W, 3))" % (image.shape,))
        h, w = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        keep = [np.ascontiguousarray(guides["node"], dtype=np.int32), np.ascontiguousarray(guides["normal"], dtype=np.float64),
                np.ascontiguousarray(guides["p"], dtype=np.float64), np.ascontiguousarray(variance, dtype=np.float32)]
        for a, shape, name in zip(keep, ((h, w), (h, w, 3), (h, w, 3), (h, w)), ("node", "normal", "p", "variance")):
            if a.shape != shape:
                raise ValueError("denoiseVariance: %s of shape %r (expected %r)" % (name, a.shape, shape))
        g = DenoiseGuides(node=keep[0].ctypes.data, normal=keep[1].ctypes.data, p=keep[2].ctypes.data)
        if age is not None:
            age = np.ascontiguousarray(age, dtype=np.uint32)
            if age.shape != (h, w):
                raise ValueError("denoiseVariance: age of shape %r (expected %r)" % (age.shape, (h, w)))
        for name, a in (("albedo", albedo), ("base", base)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.size != image.size:
                    raise ValueError("denoiseVariance: %s of shape %r (expected %r)" % (name, a.shape, image.shape))
                keep.append(a)
                setattr(g, name, a.ctypes.data)
        o = _denoise_variance_opts(w, h, ch, levels, normal_power_log2, sigma_plane, sigma_lum, var_floor, min_age)
        out = np.empty_like(image)
        vout = np.empty((h, w), dtype=np.float32) if variance_out else None
        self._check(self._lib.c2rt_denoise_variance(self._h, C.byref(g), C.byref(o), keep[3].ctypes.data_as(C.c_void_p),
                                                    None if age is None else age.ctypes.data_as(C.c_void_p), image.ctypes.data_as(C.c_void_p),
                                                    out.ctypes.data_as(C.c_void_p), None if vout is None else vout.ctypes.data_as(C.c_void_p)))
        return out, vout

    def denoiseVarianceDevice(self, ptrs, width, height, variance_ptr, age_ptr, in_ptr, out_ptr, variance_out_ptr, scratch_ptr, channels=3, levels=5,
                              normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE, sigma_lum=DENOISE_SIGMA_LUM, var_floor=DENOISE_VAR_FLOOR,
                              min_age=DENOISE_MIN_AGE, stream=0):
        """Enqueue the variance-guided filter on `stream` over device memory (c2rt_denoise_variance_device): `ptrs` as for
        denoiseDevice; age_ptr and variance_out_ptr may be 0; `scratch_ptr`: denoise_variance_scratch_bytes(...) bytes,
        16-byte aligned (0 where that is 0).  No sync; writes only out_ptr, variance_out_ptr and scratch_ptr."""
        g = DenoiseGuides()
        for n, ptr in dict(ptrs).items():
            if n not in ("node", "normal", "p", "albedo", "base"):
                raise ValueError("unknown denoise guide %r (one of node, normal, p, albedo, base)" % (n,))
            setattr(g, n, ptr or None)
        o = _denoise_variance_opts(width, height, channels, levels, normal_power_log2, sigma_plane, sigma_lum, var_floor, min_age)
        self._check(self._lib.c2rt_denoise_variance_device(self._h, C.byref(g), C.byref(o), C.c_void_p(variance_ptr or None), C.c_void_p(age_ptr or None),
                                                           C.c_void_p(in_ptr or None), C.c_void_p(out_ptr or None), C.c_void_p(variance_out_ptr or None),
                                                           C.c_void_p(scratch_ptr or None), C.c_void_p(stream)))

    def renderPathsSequenceVariance(self, cams, opts, paths, bounces, seed=0, max_age=TEMPORAL_MAX_AGE, min_normal_dot=TEMPORAL_MIN_NORMAL_DOT,
                                    max_plane_dist=TEMPORAL_MAX_PLANE_DIST, levels=5, normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE,
                                    sigma_lum=DENOISE_SIGMA_LUM, var_floor=DENOISE_VAR_FLOOR, min_age=DENOISE_MIN_AGE):
        """renderPathsSequence with the loop closed (c2rt_render_paths_sequence_variance): temporalAccumulate also writes
        its variance and age planes and the filter is denoiseVariance(..., albedo=albedo, base=rgb), fed by them; (n,
        height, width, 3) float32, bit for bit that composition."""
        cams = list(cams)
        arr = (CameraFrame * max(len(cams), 1))(*cams)
        g = _path_opts(paths, bounces, seed)
        t = _temporal_opts(opts.width, opts.height, 3, max_age, min_normal_dot, max_plane_dist)
        d = _denoise_variance_opts(opts.width, opts.height, 3, levels, normal_power_log2, sigma_plane, sigma_lum, var_floor, min_age)
        out = np.empty((len(cams), opts.height, opts.width, 3), dtype=np.float32)
        self._check(self._lib.c2rt_render_paths_sequence_variance(self._h, arr, len(cams), C.byref(opts), C.byref(g), C.byref(t), C.byref(d),
                                                                  out.ctypes.data_as(C.c_void_p)))
        return out

    def renderPathsSequenceAdaptive(self, cams, opts, paths, bounces, seed=0, min_paths=PATH_COUNT_MIN, max_paths=None, young_paths=PATH_COUNT_YOUNG,
                                    count_min_age=PATH_COUNT_MIN_AGE, paths_per_variance=PATH_COUNT_PER_VARIANCE, max_age=TEMPORAL_MAX_AGE,
                                    min_normal_dot=TEMPORAL_MIN_NORMAL_DOT, max_plane_dist=TEMPORAL_MAX_PLANE_DIST, levels=5, normal_power_log2=5,
                                    sigma_plane=DENOISE_SIGMA_PLANE, sigma_lum=DENOISE_SIGMA_LUM, var_floor=DENOISE_VAR_FLOOR, min_age=DENOISE_MIN_AGE):
        """renderPathsSequenceVariance with the sampler in the loop (c2rt_render_paths_sequence_adaptive): frame 0 is
        traced with `young_paths` everywhere, frame i > 0 with pathCounts of history i - 1, cams[i - 1] and the counts of
        frame i - 1, through renderPathsCounted with `paths` as the cap (`max_paths` None: the cap); (n, height, width, 3)
        float32, bit for bit that composition."""
        cams = list(cams)
        arr = (CameraFrame * max(len(cams), 1))(*cams)
        g = _path_opts(paths, bounces, seed)
        t = _temporal_opts(opts.width, opts.height, 3, max_age, min_normal_dot, max_plane_dist)
        d = _denoise_variance_opts(opts.width, opts.height, 3, levels, normal_power_log2, sigma_plane, sigma_lum, var_floor, min_age)
        pc = _path_count_opts(min_paths, paths if max_paths is None else max_paths, young_paths, count_min_age, paths_per_variance, young_paths)
        out = np.empty((len(cams), opts.height, opts.width, 3), dtype=np.float32)
        self._check(self._lib.c2rt_render_paths_sequence_adaptive(self._h, arr, len(cams), C.byref(opts), C.byref(g), C.byref(t), C.byref(d), C.byref(pc),
                                                                  out.ctypes.data_as(C.c_void_p)))
        return out

    def testVisibility(self, segments):
        """Scene.testVisibility for (n, 6) float64 segments (from, to): (n,) uint8, 1 = nothing in between."""
        seg = _rays_array(segments, "segments")
        vis = np.empty(seg.shape[0], dtype=np.uint8)
        self._check(self._lib.c2rt_test_visibility(self._h, seg.ctypes.data_as(C.c_void_p), seg.shape[0], vis.ctypes.data_as(C.c_void_p)))
        return vis

    def testVisibilityDevice(self, segments_ptr, n, visible_ptr, stream=0):
        """Enqueue n visibility tests on `stream`: n c2rt_segment at segments_ptr, n bytes at visible_ptr."""
        self._check(self._lib.c2rt_test_visibility_device(self._h, C.c_void_p(segments_ptr), int(n), C.c_void_p(visible_ptr), C.c_void_p(stream)))

    def deinterleaveStrips(self, gathered_ptr, frame_ptr, width, height, strip_height, world, stream=0):
        self._check(self._lib.c2rt_deinterleave_strips(self._h, C.c_void_p(gathered_ptr), C.c_void_p(frame_ptr), width, height,
                                                       strip_height, world, C.c_void_p(stream)))

    def renderFrameRGB32(self, cam, opts, stop_flag=None):
        """Blocking render in display format: (local_rows, W) uint32 0x00RRGGBB (Color.toRGB32)."""
        out = np.empty((self.localRows(opts), opts.width), dtype=np.uint32)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self._check(self._lib.c2rt_render_frame_rgb32(self._h, C.byref(cam), C.byref(opts), out.ctypes.data_as(C.c_void_p), stop))
        return out

    def renderFrameRGB32Into(self, cam, opts, out, stop_flag=None):
        """Same into a caller-owned (local_rows, W) uint32 array (pin it with pinHostBuffer for overlapped copies)."""
        assert out.dtype == np.uint32 and out.flags["C_CONTIGUOUS"] and out.size == self.localRows(opts) * opts.width
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self._check(self._lib.c2rt_render_frame_rgb32(self._h, C.byref(cam), C.byref(opts), out.ctypes.data_as(C.c_void_p), stop))
        return out

    def deinterleaveStripsRGB32(self, gathered_ptr, frame_ptr, width, height, strip_height, world, stream=0):
        self._check(self._lib.c2rt_deinterleave_strips_rgb32(self._h, C.c_void_p(gathered_ptr), C.c_void_p(frame_ptr), width, height,
                                                             strip_height, world, C.c_void_p(stream)))

    def encodeRGB32(self, frame_ptr, out_ptr, n_pixels, stream=0):
        self._check(self._lib.c2rt_encode_rgb32(self._h, C.c_void_p(frame_ptr), C.c_void_p(out_ptr), int(n_pixels), C.c_void_p(stream)))


class Renderer:
    """struct Renderer (rt/renderer.d:59-81) with the GPU behind renderRT."""

    def __init__(self, scene, ctx=None):
        self.scene = scene
        self.ctx = ctx if ctx is not None else Context()
        self._lib = _abi.load_library()

    def renderRT(self, stop_flag=None):
        s = self.scene.settings
        out = np.empty((s.frame_height, s.frame_width, 3), dtype=np.float32)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        self.ctx._check(self._lib.c2rt_host_render_rt(self.ctx.handle, self.scene._h, out.ctypes.data_as(C.c_void_p), stop))
        return out

    def renderRTAdaptive(self):
        """Context.renderFrameAdaptive for the scene's own camera and frame size at the reference's threshold
        (c2rt_host_render_rt_adaptive): (frame, mask).  A camera with depth of field or stereo is refused."""
        s = self.scene.settings
        frame = np.empty((s.frame_height, s.frame_width, 3), dtype=np.float32)
        mask = np.empty((s.frame_height, s.frame_width), dtype=np.uint8)
        self.ctx._check(self._lib.c2rt_host_render_rt_adaptive(self.ctx.handle, self.scene._h, frame.ctypes.data_as(C.c_void_p),
                                                               mask.ctypes.data_as(C.c_void_p)))
        return frame, mask

    def renderRTTaps(self, taps):
        """Context.renderFrameTaps for the scene's own camera and frame size (c2rt_host_render_rt_taps)."""
        s = self.scene.settings
        out = np.empty((s.frame_height, s.frame_width, 3), dtype=np.float32)
        self.ctx._check(self._lib.c2rt_host_render_rt_taps(self.ctx.handle, self.scene._h, C.byref(_tap_table(taps)), out.ctypes.data_as(C.c_void_p)))
        return out

    def renderRTAdaptiveTaps(self, taps):
        """Context.renderFrameAdaptiveTaps for the scene's own camera and frame size at the reference's threshold
        (c2rt_host_render_rt_adaptive_taps): (frame, mask)."""
        s = self.scene.settings
        frame = np.empty((s.frame_height, s.frame_width, 3), dtype=np.float32)
        mask = np.empty((s.frame_height, s.frame_width), dtype=np.uint8)
        self.ctx._check(self._lib.c2rt_host_render_rt_adaptive_taps(self.ctx.handle, self.scene._h, C.byref(_tap_table(taps)),
                                                                    frame.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p)))
        return frame, mask

    def renderSceneAsync(self, out, is_rendering, needs_rendering=None):
        """renderSceneAsync (rt/renderer.d:23-44); `out`, flags: numpy arrays kept alive by the caller."""
        stop = needs_rendering.ctypes.data_as(C.c_void_p) if needs_rendering is not None else None
        self.ctx._check(self._lib.c2rt_host_render_scene_async(self.ctx.handle, self.scene._h, out.ctypes.data_as(C.c_void_p),
                                                               is_rendering.ctypes.data_as(C.c_void_p), stop))

    def wait(self):
        self.ctx._check(self._lib.c2rt_host_render_wait(self.scene._h))

    def renderPixelNoAA(self, x, y):
        r = TraceResult()
        self.ctx._check(self._lib.c2rt_host_render_pixel(self.ctx.handle, self.scene._h, int(x), int(y), C.byref(r)))
        return r


    def renderHits(self, planes=("node", "leaf", "dist", "uv", "p", "normal", "rgb")):
        """Context.renderHits for the scene's own camera and frame size (c2rt_host_render_hits); a camera with depth
        of field or stereo is refused (C2rtError, ERR_UNSUPPORTED)."""
        s = self.scene.settings
        pl, out = _HIT.new(planes, (s.frame_height, s.frame_width))
        self.ctx._check(self._lib.c2rt_host_render_hits(self.ctx.handle, self.scene._h, C.byref(pl)))
        return out

    def renderHitLayers(self, max_layers, planes=("node", "leaf", "dist", "uv", "p", "normal", "rgb")):
        """Context.renderHitLayers for the scene's own camera and frame size (c2rt_host_render_hit_layers)."""
        s, K = self.scene.settings, int(max_layers)
        pl, out = _HIT.new(planes, (max(K, 0) * s.frame_height, s.frame_width))
        count = np.zeros((s.frame_height, s.frame_width), dtype=np.uint8)
        self.ctx._check(self._lib.c2rt_host_render_hit_layers(self.ctx.handle, self.scene._h, K, C.byref(pl), count.ctypes.data_as(C.c_void_p)))
        out = {k: v.reshape((K, s.frame_height) + v.shape[1:]) for k, v in out.items()}
        out["count"] = count
        return out

    def renderShading(self, planes=tuple(SHADE_PLANES)):
        """Context.renderShading for the scene's own camera and frame size (c2rt_host_render_shading)."""
        s = self.scene.settings
        pl, out = _SHADE.new(planes, (s.frame_height, s.frame_width))
        self.ctx._check(self._lib.c2rt_host_render_shading(self.ctx.handle, self.scene._h, C.byref(pl)))
        return out

    def renderOcclusion(self, samples, radius, seed=0, planes=tuple(OCCLUSION_PLANES)):
        """Context.renderOcclusion for the scene's own camera and frame size (c2rt_host_render_occlusion)."""
        s = self.scene.settings
        occ = _occlusion_opts(samples, radius, seed)
        pl, out = _OCCLUSION.new(planes, (s.frame_height, s.frame_width))
        self.ctx._check(self._lib.c2rt_host_render_occlusion(self.ctx.handle, self.scene._h, C.byref(occ), C.byref(pl)))
        return out

    def renderGather(self, samples, seed=0, planes=tuple(GATHER_PLANES)):
        """Context.renderGather for the scene's own camera and frame size (c2rt_host_render_gather)."""
        s = self.scene.settings
        g = _gather_opts(samples, seed)
        pl, out = _GATHER.new(planes, (s.frame_height, s.frame_width))
        self.ctx._check(self._lib.c2rt_host_render_gather(self.ctx.handle, self.scene._h, C.byref(g), C.byref(pl)))
        return out

    def renderPaths(self, paths=None, bounces=None, seed=0, planes=tuple(PATH_PLANES)):
        """Context.renderPaths for the scene's own camera and frame size (c2rt_host_render_paths): renderSampleGI's
        frame (rt/renderer.d:289-301) as the `radiance` plane.  None takes the scene's own pathsPerPixel / maxTraceDepth;
        a setting beyond the library's limits is refused by the library (C2rtError, ERR_LIMIT)."""
        s = self.scene.settings
        g = _path_opts(s.paths_per_pixel if paths is None else paths, s.max_trace_depth if bounces is None else bounces, seed)
        pl, out = _PATHS.new(planes, (s.frame_height, s.frame_width))
        self.ctx._check(self._lib.c2rt_host_render_paths(self.ctx.handle, self.scene._h, C.byref(g), C.byref(pl)))
        return out

    def renderPathsDenoised(self, paths=None, bounces=None, seed=0, levels=5, normal_power_log2=5, sigma_plane=DENOISE_SIGMA_PLANE, sigma_colour=0.0):
        """Context.renderPathsDenoised for the scene's own camera and frame size (c2rt_host_render_paths_denoised); None
        takes the scene's own pathsPerPixel / maxTraceDepth, as renderPaths does."""
        s = self.scene.settings
        g = _path_opts(s.paths_per_pixel if paths is None else paths, s.max_trace_depth if bounces is None else bounces, seed)
        d = _denoise_opts(s.frame_width, s.frame_height, 3, levels, normal_power_log2, sigma_plane, sigma_colour)
        out = np.empty((s.frame_height, s.frame_width, 3), dtype=np.float32)
        self.ctx._check(self._lib.c2rt_host_render_paths_denoised(self.ctx.handle, self.scene._h, C.byref(g), C.byref(d), out.ctypes.data_as(C.c_void_p)))
        return out


def renderPixel(scene, x, y, ctx=None):
    """renderPixel (rt/renderer.d:46-57): returns the TraceResult incl. colour."""
    return Renderer(scene, ctx).renderPixelNoAA(x, y)


def loadBmpImage(data):
    """loadBmpImage!Color (imageio/bmp.d:31-34): bytes -> (H, W, 3) float32."""
    lib = _abi.load_library()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    w, h = C.c_uint32(), C.c_uint32()
    p = C.POINTER(C.c_float)()
    st = lib.c2rt_host_bmp_decode(buf, len(data), C.byref(w), C.byref(h), C.byref(p))
    if st != _abi.OK:
        raise C2rtError(st, "BMP decode failed")
    arr = np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    lib.c2rt_host_free(p)
    return arr


def saveBmp(rgb):
    """Bitmap.saveImage -> saveBmp (imageio/bmp.d:195-237): (H, W, 3) float32 -> bytes."""
    lib = _abi.load_library()
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t()
    st = lib.c2rt_host_bmp_encode(rgb.ctypes.data_as(C.c_void_p), rgb.shape[1], rgb.shape[0], C.byref(out), C.byref(n))
    if st != _abi.OK:
        raise C2rtError(st, "BMP encode failed")
    data = bytes(bytearray(out[: n.value]))
    lib.c2rt_host_free(out)
    return data

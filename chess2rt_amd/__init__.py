"""chess2rt_amd — MI355X-native render hot path for Chess2RT.

Hand-written HIP kernels (gfx950) behind a plain-C ABI (include/c2rt.h), with
the reference's Scene / Camera / Renderer API mirrored in C++
(include/c2rt_host.h) and exposed here through ctypes.  No CPU fallback.
"""
from . import _abi
from ._abi import (CameraFrame, DenoiseGuides, DenoiseOpts, DenoiseVarianceOpts, GatherOpts, GatherPlanes, HostCamera, HostSettings, OcclusionOpts, OcclusionPlanes, PathCountOpts, PathOpts, PathPlanes, Ray, RayHit, RayStats, RenderOpts, SceneDesc, ScenePose, Segment,
                   ShadePlanes, TapTable, TemporalGuides, TemporalMotion, TemporalOpts, TemporalPlanes, TraceResult, TAPS_1, TAPS_4, TAPS_REF5)
from .api import (GATHER_PLANES, OCCLUSION_PLANES, PATH_PLANES, RAY_HIT_DTYPE, SHADE_PLANES, TAPS_REF5_TABLE, TEMPORAL_PLANES, C2rtError, Context, Renderer, Scene, denoise_scratch_bytes, denoise_variance_scratch_bytes, loadBmpImage, makeMotion, makePose, parseSceneFromFile, paths_counted_scratch_bytes, renderPixel, saveBmp, tap_grid, temporal_history_bytes)
from .sharding import (StripPlan, deinterleave_strips_torch, exchange_strips_p2p, local_rows, plan_strips, render_frame_sharded)

__all__ = [
    "C2rtError", "Context", "Renderer", "Scene", "parseSceneFromFile", "renderPixel", "loadBmpImage", "saveBmp",
    "CameraFrame", "HostCamera", "HostSettings", "RayStats", "RenderOpts", "SceneDesc", "ScenePose", "makePose", "TraceResult",
    "Ray", "Segment", "RayHit", "RAY_HIT_DTYPE", "ShadePlanes", "SHADE_PLANES",
    "OcclusionOpts", "OcclusionPlanes", "OCCLUSION_PLANES",
    "GatherOpts", "GatherPlanes", "GATHER_PLANES",
    "PathOpts", "PathPlanes", "PATH_PLANES", "PathCountOpts", "paths_counted_scratch_bytes",
    "DenoiseGuides", "DenoiseOpts", "denoise_scratch_bytes", "DenoiseVarianceOpts", "denoise_variance_scratch_bytes",
    "TemporalGuides", "TemporalMotion", "TemporalOpts", "TemporalPlanes", "TEMPORAL_PLANES", "temporal_history_bytes", "makeMotion",
    "TAPS_1", "TAPS_4", "TAPS_REF5", "TapTable", "TAPS_REF5_TABLE", "tap_grid",
    "StripPlan", "plan_strips", "local_rows", "render_frame_sharded", "deinterleave_strips_torch", "exchange_strips_p2p",
]

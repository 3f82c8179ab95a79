"""GPU: shade() and light_terms() of c2rt_trace.inc, tex_color() and bitmap_filtered() of c2rt_trace_shared.inc in isolation, against
tests/shade_reference.py (a typed numpy restatement of the reference's shading stage written from the D source, which
tests/test_shade_reference.py holds against the oracle on the CPU).

Per light variant of tests/shade_scenes.py (1, 2, 4, 5 and 33 lights; a dark light and one outside 2^+-60 in the
middle), one upload: the GPU's own hit records and its own visibility answers go INTO the reference, and the colour
that comes out must have the bits of the GPU's colour on every sample that is not ambiguous (a pow / sin value within
4 fp64 ulp of a float32 rounding midpoint); an ambiguous sample must lie within the bounds of its re-evaluations.
No tolerance anywhere."""
import functools

import numpy as np
import pytest

import oracle_lib as orc
import shade_reference as sr
import shade_scenes as ss
from golden_configs import SCENES
from ray_query_util import oracle_visibility

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 0.001
_gpu_cases = {}


def gpu_case(gpu_ctx, variant):
    """uploads the variant and returns {ray set: (rays, GPU records, GPU rgb, GPU visibility, reference Shaded)} — the
    queries run once per variant and are shared by the tests below (read-only)"""
    scene, _, _ = ss.load(variant)
    gpu_ctx.uploadScene(scene.desc)
    if variant not in _gpu_cases:
        T = sr.Tables(scene.desc)
        lit = T.lit()
        out = {}
        for name in ss.RAY_SETS:
            rays = ss.ray_set(variant, name)
            rec, rgb = gpu_ctx.traceRays(rays)
            segs = sr.shadow_segments(T, rays[:, 3:], rec).reshape(len(rays), T.n_lights, 6)
            hit = rec["closest_node"] >= 0
            ask = np.ascontiguousarray(segs[hit][:, lit].reshape(-1, 6))        # every lit light of every hit
            vis = np.zeros((len(rays), T.n_lights), dtype=np.uint8)
            got = gpu_ctx.testVisibility(ask)
            sub = np.zeros((int(hit.sum()), T.n_lights), dtype=np.uint8)
            sub[:, lit] = got.reshape(-1, int(lit.sum()))
            vis[hit] = sub
            out[name] = (rays, rec, rgb, vis, ask, got, sr.shade(T, rays[:, 3:], rec, vis))
        _gpu_cases[variant] = out
    return _gpu_cases[variant]


@pytest.mark.parametrize("variant", ss.VARIANTS)
def test_query_colours_equal_the_reference_of_the_gpus_own_records(gpu_ctx, variant):
    scene, _, _ = ss.load(variant)
    for name, (rays, rec, rgb, vis, ask, got, ref) in gpu_case(gpu_ctx, variant).items():
        assert np.array_equal(got, oracle_visibility(scene.desc, ask)), (variant, name, "visibility differs from the oracle")
        plain, outside = sr.compare(rgb, ref)
        print("%s %s: %d samples, %d near a midpoint, %d tiny sines, %d floats differ outside the ambiguous, %d outside their bounds"
              % (variant, name, len(rays), ref.midpoint.sum(), ref.tiny.sum(), plain, outside))
        assert ref.midpoint.sum() <= AMBIGUOUS_CAP * len(rays), (variant, name)
        assert plain == 0 and outside == 0, (variant, name, plain, outside)
        # a tiny sine has no neighbouring cast: those samples are bit-equal as well
        only_tiny = ref.tiny & ~ref.midpoint
        assert np.array_equal(rgb[only_tiny].view(np.uint32), ref.rgb[only_tiny].view(np.uint32)), (variant, name)


def light_leaves_the_lean_window(T):
    """a lit light with a channel that is neither +0 nor within 2^+-60 (DevLight::lit bit 1 clear)"""
    c = np.abs(T.light_colors()[T.lit()])
    return bool(((c != 0) & ((c < 2.0 ** -60) | (c >= 2.0 ** 60))).any())


@pytest.mark.parametrize("variant", ss.VARIANTS)
def test_frame_and_batch_equal_the_reference_of_the_screen_rays(gpu_ctx, variant):
    """renderFrame runs the lean:: instance (culling masks, light_shadow_mask, the fp32 lean division)"""
    scene, cam, opts = ss.load(variant)
    rays, rec, rgb, vis, _, _, ref = gpu_case(gpu_ctx, variant)["screen"]
    before = gpu_ctx.exactRedos()
    frame = gpu_ctx.renderFrame(cam, opts)
    redone = gpu_ctx.exactRedos() - before
    plain, outside = sr.compare(frame, ref)
    print("%s frame: %d tiles redone exactly, %d floats differ outside the ambiguous, %d outside their bounds" % (variant, redone, plain, outside))
    assert plain == 0 and outside == 0, (variant, plain, outside)
    T = sr.Tables(scene.desc)
    if variant in ("L1", "L2"):
        assert redone == 0, "the lean instance handed tiles to the exact one"
        assert not light_leaves_the_lean_window(T)
    if variant in ("L4", "L5"):
        # the fallback of `lit` bit 1 is a per-light branch inside lean::, not a tile redo: what shows it is that a lit
        # light outside the window is on the list, lights some screen sample, and the frame still has the reference's bits
        l = 3
        assert redone > 0 or (light_leaves_the_lean_window(T) and int(vis[:, l].sum()) >= 30)
    batch = gpu_ctx.renderFrames([cam, cam, cam], opts)
    assert np.array_equal(batch[1].view(np.uint32), frame.view(np.uint32)), variant


@functools.lru_cache(maxsize=None)
def _lecture4():
    import chess2rt_amd as c2
    import os

    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture4.sdl"))
    scene.setFrameSize(160, 120)
    scene.setDof(False)
    return scene


@pytest.mark.parametrize("which", ["lecture4", "L1_without_phong_and_procedure2"])
@pytest.mark.parametrize("taps", [1, 5])
def test_libm_free_scenes_are_bit_identical_to_the_oracle(gpu_ctx, which, taps):
    """no pow, no sin, no textured sphere: nothing but IEEE operations on the path, so every bit is asserted"""
    scene = _lecture4() if which == "lecture4" else ss.load("L1", True)[0]
    scene.setAA(taps == 5)
    cam = scene.beginFrame()
    opts = scene.renderOpts(taps=taps)
    gpu_ctx.uploadScene(scene.desc)
    gpu = gpu_ctx.renderFrame(cam, opts)
    ref = orc.render_frame(scene.desc, cam, opts, 0)
    scene.setAA(False)
    assert np.array_equal(gpu.view(np.uint32), ref.view(np.uint32)), (which, taps, int((gpu.view(np.uint32) != ref.view(np.uint32)).sum()))

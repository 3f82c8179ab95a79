"""The three PARTS of the reference's shade() — diffuseColor, lightContrib, Phong's specular — from tests/shade_reference.py
(imported, not edited) called on copies of its Tables with fields replaced, for the shading planes' tests
(tests/test_shade_planes_abi.py on the CPU, tests/test_gpu_shade_planes.py on the GPU).

  light     every shader Lambert, no texture, colour (1, 1, 1): sr.shade returns 1 * lightContrib, which is lightContrib
            bit for bit.  No pow and no sin is on that path (asserted: libm_calls == 0).
  specular  no textures, every colour (0, 0, 0), shader types kept: sr.shade returns (0 * lightContrib) + specular for a
            Phong node and 0 * lightContrib for a Lambert node.  0 * x is +0 while x is finite and not negative
            (asserted on `light`), and +0 + specular is specular (a sum that starts at +0 is never -0).
  albedo    the original tables with nothing visible and ambient (1, 1, 1): sr.shade returns (diffuse * 1) + (+0),
            which is diffuse (no texture or colour of the scenes used is -0).

Each part is a shade_reference.Shaded: values, the ambiguous samples (a pow / sin value near a float32 rounding midpoint)
and their bounds, for shade_reference.compare.  Misses are +0 in every part."""
import copy

import numpy as np

import shade_reference as sr

F32 = np.float32


def light_tables(T):
    t = copy.copy(T)
    t.shader_type = np.full_like(T.shader_type, sr.SHADER_LAMBERT)
    t.shader_texture = np.full_like(T.shader_texture, -1)
    t.shader_color = np.ones_like(T.shader_color)
    return t


def specular_tables(T):
    t = copy.copy(T)
    t.shader_texture = np.full_like(T.shader_texture, -1)
    t.shader_color = np.zeros_like(T.shader_color)
    return t


def albedo_tables(T):
    t = copy.copy(T)
    t.ambient = np.ones(3, dtype=F32)
    return t


class Parts:
    """albedo, light, specular: shade_reference.Shaded | phong, hit: (n,) bool"""


def parts(T, dirs, recs, vis):
    """the three parts of shade() of every record, for the visibility answers `vis` (n, n_lights)"""
    n = len(recs)
    vis = np.asarray(vis).reshape(n, -1)
    r = Parts()
    r.hit = recs["closest_node"] >= 0
    r.phong = np.zeros(n, dtype=bool)
    r.phong[r.hit] = T.shader_type[T.node_shader[recs["closest_node"][r.hit]]] == sr.SHADER_PHONG
    r.light = sr.shade(light_tables(T), dirs, recs, vis)
    assert r.light.libm_calls == 0 and not r.light.ambiguous.any()
    # what makes 0 * lightContrib a +0 below
    assert np.isfinite(r.light.rgb).all() and not np.signbit(r.light.rgb).any()
    r.specular = sr.shade(specular_tables(T), dirs, recs, vis)
    r.albedo = sr.shade(albedo_tables(T), dirs, recs, np.zeros_like(vis))
    return r


def recombine(albedo, light, specular, phong):
    """shade's last statements in float32: diffuse * lightContrib, + specular for a Phong node (shader.d:104, 249)"""
    albedo, light, specular = (np.ascontiguousarray(a, dtype=F32).reshape(-1, 3) for a in (albedo, light, specular))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        res = albedo * light
        return np.where(np.asarray(phong).reshape(-1)[:, None], res + specular, res).astype(F32)


def same_bits(a, b):
    """(n, 3) bool: equal bits, NaN equal to NaN"""
    a, b = (np.ascontiguousarray(x, dtype=F32).reshape(-1, 3) for x in (a, b))
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def pack_visible(T, vis):
    """the `visible` plane of (n, n_lights) visibility answers: bit l for the lit lights l < 32"""
    vis = np.asarray(vis).astype(bool)
    lit = T.lit()
    word = np.zeros(len(vis), dtype=np.uint32)
    for l in range(min(T.n_lights, 32)):
        if lit[l]:
            word |= vis[:, l].astype(np.uint32) << np.uint32(l)
    return word

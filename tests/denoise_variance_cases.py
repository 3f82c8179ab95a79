"""Shared by tests/test_denoise_variance_abi.py (CPU) and tests/test_gpu_denoise_variance.py (GPU): the synthetic frames of
tests/test_gpu_denoise.py restated, the edge values injected into a variance plane, and the options both halves use, so
that what the CPU half shows not to be vacuous is what the GPU half compares."""
import numpy as np

MIN_AGE = 3                    # with the four-frame sequences of temporal_cases: frame 3 holds ages 1 .. 4
SIGMA_LUM = 4.0
VAR_FLOOR = 1e-8
TINY_FLOOR = 1e-45             # a subnormal: 1f / (0 + it) overflows to +inf, and every tap with dl != 0 is dropped
MAX_AGE = 8


def synthetic(h, w, seed, channels=3):
    """tests/test_gpu_denoise.py's: a few nodes in patches and misses among them, normals scattered about +z, points near
    a plane; and with them a variance of the image's order and ages on both sides of MIN_AGE"""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    node = (((xs // 5) + 2 * (ys // 3)) % 3).astype(np.int32)
    node[rng.uniform(size=(h, w)) < 0.1] = -1
    normal = rng.uniform(-0.6, 0.6, (h, w, 3))
    normal[..., 2] = 1.0
    normal[rng.uniform(size=(h, w)) < 0.05] *= -1.0
    p = np.stack([xs * 0.25, ys * 0.25, rng.uniform(-0.5, 0.5, (h, w))], axis=-1)
    img = rng.uniform(0.0, 2.0, (h, w, channels)).astype(np.float32)
    variance = rng.uniform(0.0, 0.3, (h, w)).astype(np.float32)
    age = rng.randint(0, 2 * MIN_AGE + 1, (h, w)).astype(np.uint32)
    return dict(node=node, normal=normal, p=p), img, variance, age


def noise_indirect(seed, h, w):
    """the seeded `indirect` of the CPU half's sequences: log-normal, exp(N(-1, 1)), median 0.37 with a long tail — the
    fireflies of a path tracer.  A bounded noise (uniform: at most 1.7 standard deviations off its mean) cannot put a tap
    four standard deviations off before smoothing and leaves level 0's luminance term idle."""
    return np.random.RandomState(seed).lognormal(-1.0, 1.0, (h, w, 3)).astype(np.float32)


def inject(variance, node):
    """a copy of `variance` with, on hit pixels spread over the frame: NaN (every tap of the 3x3 around it is dropped, and
    the pixels that keep it as a tap take it into V'), +inf (inv_l = 0: the term is off), a negative value, and a patch of
    zeros (where TINY_FLOOR alone holds the term)"""
    v = np.array(variance, dtype=np.float32, copy=True)
    h, w = v.shape
    ys, xs = np.nonzero(np.asarray(node) >= 0)
    pick = np.random.RandomState(7).permutation(ys.size)
    for k, value in zip(pick[:12], [np.nan] * 6 + [np.inf] * 3 + [-0.5] * 3):
        v[ys[k], xs[k]] = value
    v[h // 3:h // 3 + 8, w // 3:w // 3 + 10] = 0.0
    return v

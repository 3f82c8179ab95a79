"""A typed restatement of the reference's CAMERA and SAMPLING stages, independent of oracle/c2rt_oracle.c and of the
device code: the third sibling of tests/geom_reference.py and tests/shade_reference.py.  With them a whole frame is
computed with no oracle in it: camera -> rays (`begin_frame`, `screen_ray`) -> records (gr.trace) -> visibility
(gr.test_visibility) -> colour (sr.shade) -> pixel (`render_frame`).

Written from the reference's D source (paths relative to its source/rt/): camera.d:77-117 (beginFrame), 231-236
(setFrameSize), 252 (discMultiplier = 10.0 / fNumber), 123-174 (getScreenRay), 258-269 (unitDiscSample),
renderer.d:110-127 (the pre-pass blocks), 194-213 (buckets and their clip), 223-251 (renderPixelNoAA, renderPixelAA),
254-313 (renderSample, renderSampleDof, renderSampleDefault), color.d:10-15 (combineStereo), 77-83 (adjustSaturation),
128-132 (Color / float divides; opOpAssign!"/" would multiply by a reciprocal), 141-144 (intensity) and
imported_types.d:13-20 (mul).  gfm:math is not part of the reference's tree; its published algorithms are used:
radians is `x * (PI / 180)` with std.math's 80-bit PI, mat3d.rotateX / rotateY / rotateZ are rotateAxis!(1, 2), !(2, 0),
!(0, 1) (identity, then c[i][i] = cos, c[i][j] = -sin, c[j][i] = sin, c[j][j] = cos), the matrix product is
`sum = 0; sum += c[i][k] * x.c[k][j]`, magnitude is sqrt of `sum = 0; sum += v_i * v_i`, normalize is
`v *= 1 / sqrt(squaredMagnitude)`, vector * scalar is component by component.

What the reference leaves irreproducible is BUILD-DEFINED and restated from its specification (DESIGN.md section 2 and
the comments above hash32 and lens_sincos2pi in chess2rt_amd/csrc/c2rt_trace_shared.inc), not from its code:
  - uniform(0, 1) is a counter-based RNG: hash32 is the 32-bit multiply-xorshift finaliser "lowbias32" (shifts 16, 15,
    16; multipliers 0x7feb352d, 0x846ca68b); the key folds the seed's high word (xor 0x243f6a88), its low word (xor),
    the pixel's high word (add), its low word (xor) and the tap (add), one hash each; a draw is
    hash32(key + 0x9e3779b9 * (16 * sample + dim + 1)) * 2^-32.  `pixel` is frame row * W + column of the pixel the
    sample is taken FOR (under prepass_bucket: the block's corner); `sample` is the lens sample, `dim` counts the draws
    within it, in the reference's order: per eye x jitter, y jitter (renderer.d:277-282, arguments left to right), then
    unitDiscSample's angle and radius (camera.d:265-266);
  - (sin, cos)(2 pi u): t = 4u, quadrant q = int(t), f = t - q, mirrored about 0.5 to g; theta = g * (pi / 2 as a
    double); Taylor polynomials in theta, sin to theta^17 and cos to theta^16, by Horner in z = theta^2 with the
    coefficients +-1/k! correctly rounded, closed as theta + theta * (z * P) and 1 + z * Q; a mirrored pair is swapped;
    the quadrant rotates (a, b) -> (b, -a) -> (-a, -b) -> (-b, a);
  - C2RT_TAPS_4: the first four entries of the 5-tap table, sum / 4 (include/c2rt.h);
  - interleaved strips and prepass_bucket as c2rt_render_opts documents them.

Rules of evaluation:
  - every operation in the type the D source gives it, in source order, nothing fused (numpy never contracts): camera
    and ray arithmetic in np.float64, Color arithmetic in np.float32; `average / numSamples` and `accum / 5` narrow the
    integer to float and DIVIDE, per channel;
  - radians is formed in np.longdouble (x87: 64-bit significand, asserted by `require_x87`) and rounded once;
  - tan, sin, cos of beginFrame come from mpmath at 50 digits, rounded once to double;
  - `a + b * s + c * t` is ((a + b * s) + c * t); mul(v, m) is a ROW vector times c[i][j];
  - a sample whose pow or sin lies at a float32 rounding midpoint has a per-channel range (sr.shade).  fp32 addition,
    multiplication by a non-negative constant and division by a positive constant are monotone, so the low and the high
    end are carried through combineStereo and both sums; `compare` holds a pixel to its bits where the range is one
    float and no sample of it is flagged, and to [lo, hi] elsewhere.  No pixel is left out.

Vectorised over every ray of a frame at once."""
import math
from fractions import Fraction

import mpmath
import numpy as np

import geom_reference as gr
import shade_reference as sr

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
LD = np.longdouble
TAPS_1, TAPS_REF5, TAPS_4 = 1, 5, 4          # c2rt_tap_mode, include/c2rt.h
AA_KERNEL = ((0.0, 0.0), (0.3, 0.3), (0.6, 0.0), (0.0, 0.6), (0.6, 0.6))      # renderer.d:235-242
LEFT, NONE, RIGHT = -1, 0, +1                # Stereo3DOffset

# the named misreadings of test_camera_reference's mutation check (each changes ONE statement below)
MUTATIONS = ("pixel_centre", "aspect_inverted", "rotation_order_reversed", "column_vector_product", "fov_not_halved",
             "second_stereo_offset_dropped", "stereo_sign_swapped", "lens_sin_cos_swapped", "disc_multiplier_is_fnumber",
             "focal_distance_along_ray", "cos_from_unnormalised_dir", "lens_up_before_right", "taps_two_and_three_swapped",
             "tap_divide_by_reciprocal", "eyes_share_one_jitter", "draws_lens_before_jitter", "rng_pixel_from_local_row",
             "prepass_block_not_clipped", "prepass_pixel_from_own_xy", "saturation_after_channel_mask")

_MP = mpmath.mp.clone()
_MP.dps = 50


def _to_double(x):
    return mpmath.libmp.to_float(x._mpf_, rnd=mpmath.libmp.round_nearest)


def x87_available():
    return np.finfo(LD).nmant == 63


def require_x87():
    assert x87_available(), "np.longdouble is not the x87 80-bit format here"


# ---- gfm:math ---------------------------------------------------------------------------------------------------------------


def radians(deg):
    """gfm radians!double: x * (PI / 180), the constant folded and the product formed in 80 bits, rounded once"""
    require_x87()
    pi = LD("3.14159265358979323846264338327950288419716939937510")
    return F64(LD(F64(deg)) * (pi / LD(180)))


def _libm(fn, x):
    return F64(_to_double(getattr(_MP, fn)(_MP.mpf(float(x)))))


def rotate_axis(i, j, angle):
    m = np.zeros((3, 3), dtype=F64)
    m[0, 0] = m[1, 1] = m[2, 2] = 1.0
    cosa, sina = _libm("cos", angle), _libm("sin", angle)
    m[i, i] = cosa
    m[i, j] = -sina
    m[j, i] = sina
    m[j, j] = cosa
    return m


def rotate_x(a):
    return rotate_axis(1, 2, a)


def rotate_y(a):
    return rotate_axis(2, 0, a)


def rotate_z(a):
    return rotate_axis(0, 1, a)


def matmul(a, b):
    r = np.zeros((3, 3), dtype=F64)
    for i in range(3):
        for j in range(3):
            s = F64(0)
            for k in range(3):
                s = s + a[i, k] * b[k, j]
            r[i, j] = s
    return r


def mul(v, m, mut=None):
    """imported_types.d:13-20"""
    x, y, z = F64(v[0]), F64(v[1]), F64(v[2])
    if mut == "column_vector_product":
        return np.array([x * m[0, 0] + y * m[0, 1] + z * m[0, 2],
                         x * m[1, 0] + y * m[1, 1] + z * m[1, 2],
                         x * m[2, 0] + y * m[2, 1] + z * m[2, 2]], dtype=F64)
    return np.array([x * m[0, 0] + y * m[1, 0] + z * m[2, 0],
                     x * m[0, 1] + y * m[1, 1] + z * m[2, 1],
                     x * m[0, 2] + y * m[1, 2] + z * m[2, 2]], dtype=F64)


def dot(a, b):
    s = np.zeros(np.broadcast(a[..., 0], b[..., 0]).shape, dtype=F64)
    for i in range(3):
        s = s + a[..., i] * b[..., i]
    return s


def normalized(v):
    inv = F64(1) / np.sqrt(dot(v, v))
    return v * inv[..., None]


# ---- camera.d ---------------------------------------------------------------------------------------------------------------

FRAME_VECTORS = ("pos", "up_left", "up_right", "down_left", "right_dir", "up_dir", "front_dir")


class Frame:
    """the fields of c2rt_camera_frame (include/c2rt.h), and f_number (disc_multiplier = 10 / f_number)"""

    def __repr__(self):
        return "Frame(%s)" % ", ".join("%s=%r" % kv for kv in sorted(self.__dict__.items()))


def begin_frame(pos, yaw, pitch, roll, fov, W, H, dof=False, num_samples=25, focal_plane_dist=1.0, f_number=1.0,
                stereo_separation=0.0, mut=None):
    """setFrameSize (camera.d:231-236) then beginFrame (camera.d:77-117)"""
    fr = Frame()
    frame_width, frame_height = int(W), int(H)
    aspect = F64(frame_width) / F64(frame_height)
    if mut == "aspect_inverted":
        aspect = F64(frame_height) / F64(frame_width)
    pos = np.array(pos, dtype=F64)
    x = -aspect
    y = F64(+1)
    corner = np.array([x, y, 1.0], dtype=F64)
    center = np.array([0.0, 0.0, 1.0], dtype=F64)
    d = corner - center
    lenXY = np.sqrt(dot(d, d))
    wantedLength = _libm("tan", radians(F64(fov) if mut == "fov_not_halved" else F64(fov) / F64(2)))
    scaling = wantedLength / lenXY
    x = x * scaling
    y = y * scaling
    upLeft = np.array([x, y, 1.0], dtype=F64)
    upRight = np.array([-x, y, 1.0], dtype=F64)
    downLeft = np.array([x, -y, 1.0], dtype=F64)
    if mut == "rotation_order_reversed":
        rotation = matmul(matmul(rotate_y(radians(yaw)), rotate_x(radians(pitch))), rotate_z(radians(roll)))
    else:
        rotation = matmul(matmul(rotate_z(radians(roll)), rotate_x(radians(pitch))), rotate_y(radians(yaw)))
    upLeft = mul(upLeft, rotation, mut)
    upRight = mul(upRight, rotation, mut)
    downLeft = mul(downLeft, rotation, mut)
    fr.right_dir = mul((1.0, 0.0, 0.0), rotation, mut)
    fr.up_dir = mul((0.0, 1.0, 0.0), rotation, mut)
    fr.front_dir = mul((0.0, 0.0, 1.0), rotation, mut)
    fr.up_left = upLeft + pos
    fr.up_right = upRight + pos
    fr.down_left = downLeft + pos
    fr.pos = pos
    fr.frame_width, fr.frame_height = F64(frame_width), F64(frame_height)
    fr.dof, fr.num_samples = bool(dof), int(num_samples)
    fr.focal_plane_dist, fr.f_number = F64(focal_plane_dist), F64(f_number)
    fr.disc_multiplier = F64(10.0) / F64(f_number)                     # camera.d:252
    fr.stereo_separation = F64(stereo_separation)
    return fr


def rotate(yaw, pitch, roll, d_yaw, d_roll, d_pitch):
    """Camera.rotate, camera.d:211-229 -> (yaw, pitch, roll)"""
    yaw, roll, pitch = F64(yaw) + F64(d_yaw), F64(roll) + F64(d_roll), F64(pitch) + F64(d_pitch)
    return yaw, min(max(pitch, F64(-90)), F64(90)), roll


def move(frame, dx, dy, dz):
    """Camera.move, camera.d:181-204, with the directions the last beginFrame left -> pos"""
    pos = frame.pos + F64(dx) * frame.right_dir
    pos = pos + F64(dy) * frame.up_dir
    return pos + F64(dz) * frame.front_dir


def screen_ray(frame, x, y, offset=NONE, lens=None, mut=None):
    """getScreenRay (camera.d:123-174) for arrays x, y -> (orig (n, 3), dir (n, 3)); `lens`: unitDiscSample's two
    uniform draws (angle, radius) as arrays, read only when frame.dof"""
    x, y = np.atleast_1d(np.asarray(x, dtype=F64)), np.atleast_1d(np.asarray(y, dtype=F64))
    if mut == "pixel_centre":
        x, y = x + F64(0.5), y + F64(0.5)
    n = len(x)
    pos = frame.pos
    with np.errstate(all="ignore"):
        target = (frame.up_left + (frame.up_right - frame.up_left) * (x / frame.frame_width)[:, None]) \
            + (frame.down_left - frame.up_left) * (y / frame.frame_height)[:, None]
        raw = target - pos
        dirn = normalized(raw)
        orig = np.broadcast_to(pos, (n, 3)).copy()
        sep = frame.stereo_separation
        if mut == "stereo_sign_swapped":
            sep = -sep
        if offset != NONE:
            orig = orig + frame.right_dir * (+sep if offset == RIGHT else -sep)
        if not frame.dof:
            return orig, dirn
        cosTheta = dot(raw if mut == "cos_from_unnormalised_dir" else dirn, frame.front_dir)
        M = np.broadcast_to(frame.focal_plane_dist, (n,)) if mut == "focal_distance_along_ray" else frame.focal_plane_dist / cosTheta
        T = orig + dirn * M[:, None]
        sn, cs = lens_sincos2pi(lens[0])
        if mut == "lens_sin_cos_swapped":
            sn, cs = cs, sn
        rad = np.sqrt(np.asarray(lens[1], dtype=F64))
        dx, dy = sn * rad, cs * rad
        mult = frame.f_number if mut == "disc_multiplier_is_fnumber" else frame.disc_multiplier
        dx, dy = dx * mult, dy * mult
        if mut == "lens_up_before_right":
            orig = (pos + dy[:, None] * frame.up_dir) + dx[:, None] * frame.right_dir
        else:
            orig = (pos + dx[:, None] * frame.right_dir) + dy[:, None] * frame.up_dir
        if offset != NONE and mut != "second_stereo_offset_dropped":
            orig = orig + frame.right_dir * (+sep if offset == RIGHT else -sep)
        return orig, normalized(T - orig)


# ---- the build-defined lens sample --------------------------------------------------------------------------------------------


def hash32(x):
    x = np.asarray(x, dtype=U32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U32(16)
        x *= U32(0x7feb352d)
        x ^= x >> U32(15)
        x *= U32(0x846ca68b)
        x ^= x >> U32(16)
    return x


def rng_key(seed, pixel, tap):
    seed = U64(seed)
    pixel, tap = np.asarray(pixel, dtype=U64), np.asarray(tap, dtype=U32)
    with np.errstate(over="ignore"):
        k = hash32(U32(seed >> U64(32)) ^ U32(0x243f6a88))
        k = hash32(k ^ U32(seed & U64(0xffffffff)))
        k = hash32(k + (pixel >> U64(32)).astype(U32))
        k = hash32(k ^ (pixel & U64(0xffffffff)).astype(U32))
        return hash32(k + tap)


def rng_uniform(key, sample, dim):
    """in [0, 1): 32 random bits"""
    sample, dim = np.asarray(sample, dtype=U32), np.asarray(dim, dtype=U32)
    with np.errstate(over="ignore"):
        h = hash32(np.asarray(key, dtype=U32) + U32(0x9e3779b9) * (sample * U32(16) + dim + U32(1)))
    return h.astype(F64) * F64(2.0 ** -32)


def _inv_factorial(k):
    """1/k! correctly rounded (int / int is)"""
    f = Fraction(1, math.factorial(k))
    return F64(f.numerator / f.denominator)


SIN_COEFFS = tuple((-1) ** ((k - 1) // 2) * _inv_factorial(k) for k in (17, 15, 13, 11, 9, 7, 5, 3))    # highest first
COS_COEFFS = tuple((-1) ** (k // 2) * _inv_factorial(k) for k in (16, 14, 12, 10, 8, 6, 4, 2))
HALF_PI = F64(_to_double(_MP.pi / 2))


def lens_sincos2pi(u):
    u = np.atleast_1d(np.asarray(u, dtype=F64))
    t = u * F64(4)
    q = t.astype(np.int64)
    f = t - q.astype(F64)
    mirror = f > 0.5
    g = np.where(mirror, F64(1) - f, f)
    th = g * HALF_PI
    z = th * th
    ps = np.full(len(u), SIN_COEFFS[0])
    for c in SIN_COEFFS[1:]:
        ps = c + z * ps
    s = th + th * (z * ps)
    pc = np.full(len(u), COS_COEFFS[0])
    for c in COS_COEFFS[1:]:
        pc = c + z * pc
    c = F64(1) + z * pc
    a, b = np.where(mirror, c, s), np.where(mirror, s, c)
    odd = (q & 1) == 1
    sn, cs = np.where(odd, b, a), np.where(odd, a, b)
    sn = np.where((q == 2) | (q == 3), -sn, sn)
    cs = np.where((q == 1) | (q == 2), -cs, cs)
    return sn, cs


def exact_sincos2pi(u):
    """mpmath's (sin, cos)(2 pi u) of ONE double u, as mpf"""
    a = 2 * _MP.pi * _MP.mpf(float(u))
    return _MP.sin(a), _MP.cos(a)


# ---- renderer.d -------------------------------------------------------------------------------------------------------------------


class Opts:
    """the fields of c2rt_render_opts this stage reads"""

    def __init__(self, width, height, taps=TAPS_1, strip_height=0, strip_rank=0, strip_world=0, seed=0, prepass_bucket=0):
        self.width, self.height, self.taps = int(width), int(height), int(taps)
        self.strip_height, self.strip_rank, self.strip_world = int(strip_height), int(strip_rank), int(strip_world)
        self.seed, self.prepass_bucket = int(seed), int(prepass_bucket)


def local_frame_rows(opts):
    """the frame rows of this rank, in the order of its compact buffer: strips rank, rank + world, .. of strip_height"""
    rows = np.arange(opts.height)
    if opts.strip_world <= 1:
        return rows
    sh = opts.strip_height or 1
    return rows[(rows // sh) % opts.strip_world == opts.strip_rank]


def prepass_blocks(W, H, bucket, mut=None):
    """renderer.d:194-213 and 110-127 -> [(x0, y0, dx, dy)]: a 16x16 block clipped by its bucket, the bucket by the frame"""
    out = []
    for by in range(0, H, bucket):
        for bx in range(0, W, bucket):
            bw, bh = min(bx + bucket, W) - bx, min(by + bucket, H) - by          # bucket.clip(W, H)
            for dy in range(0, bh, 16):
                ey = min(bh, dy + 16)
                for dx in range(0, bw, 16):
                    ex = min(bw, dx + 16)
                    out.append((bx + dx, by + dy, ex - dx, ey - dy))
    return out


def adjust_saturation(c, amount):
    """color.d:77-83, intensity :141-144"""
    amount = F32(amount)
    mid = ((c[:, 0] + c[:, 1]) + c[:, 2]) / F32(3)
    rest = mid * (F32(1) - amount)
    return np.stack([c[:, k] * amount + rest for k in range(3)], axis=1).astype(F32)


def combine_stereo(left, right, mut=None):
    """color.d:10-15"""
    red, cyan = np.array([1, 0, 0], dtype=F32), np.array([0, 1, 1], dtype=F32)
    if mut == "saturation_after_channel_mask":
        return adjust_saturation(left * red, 0.25) + adjust_saturation(right * cyan, 0.25)
    return adjust_saturation(left, 0.25) * red + adjust_saturation(right, 0.25) * cyan


def accumulate(colour, ntaps, ns, ne, frame, mut=None):
    """colour (ntaps * ns * ne * S, 3) float32 in the order [tap][lens sample][eye][site] -> (S, 3): combineStereo, the
    lens loop (renderer.d:270-287), the tap loop (:233-251).  Every step is monotone in each input."""
    S = len(colour) // (ntaps * ns * ne)
    c = colour.reshape(ntaps, ns, ne, S, 3)
    accum = None
    for tap in range(ntaps):
        average = np.zeros((S, 3), dtype=F32)
        for i in range(ns):
            sample = combine_stereo(c[tap, i, 0], c[tap, i, 1], mut) if ne == 2 else c[tap, i, 0]
            if not frame.dof:
                average = sample                                    # renderSampleDefault returns it
            else:
                average = average + sample                          # renderer.d:277-283
        if frame.dof:
            average = average / F32(frame.num_samples)              # :286
        accum = average if tap == 0 else accum + average            # :244-248
    if ntaps > 1:
        accum = accum * (F32(1) / F32(ntaps)) if mut == "tap_divide_by_reciprocal" else accum / F32(ntaps)   # :249
    return accum.astype(F32)


class Rendered:
    """rgb, lo, hi (rows, W, 3) float32 | ambiguous (rows, W) bool: a sample of the pixel is flagged by sr.shade |
    wide (rows, W) bool: lo != hi in some channel | rays (n, 6), trace: gr.trace's Trace of the primary rays |
    draws: every uniform the frame drew | sample_ambiguous: the flagged share of the samples"""


def render_frame(tables, frame, opts, seed=None, mut=None):
    """Renderer.renderRT's second pass (and its AA pass for taps 5, the build's taps 4; the pre-pass alone under
    prepass_bucket) for the rows of opts' rank.  tables: (gr.Tables, sr.Tables) of one descriptor -> Rendered"""
    T, Ts = tables
    W, H = opts.width, opts.height
    seed = opts.seed if seed is None else seed
    rows = local_frame_rows(opts)
    # the sites a sample is taken for: (column, frame row, jitter extents, the pixel of the RNG key)
    if opts.prepass_bucket:
        blocks = prepass_blocks(W, H, opts.prepass_bucket)
        # (sample x, sample y, jitter extents, then the rectangle the sample is drawn over: its corner keys the RNG)
        if mut == "prepass_pixel_from_own_xy":
            sites = [(x0, y0, dx, dy, x, y, 1, 1) for x0, y0, dx, dy in blocks for y in range(y0, y0 + dy) for x in range(x0, x0 + dx)]
        else:
            sites = [(x0, y0, dx, dy, x0, y0, dx, dy) for x0, y0, dx, dy in blocks]
        sites = np.array(sites, dtype=np.int64)
        sx, sy, jdx, jdy, kx = sites[:, 0], sites[:, 1], sites[:, 2], sites[:, 3], sites[:, 4]
        if mut == "prepass_block_not_clipped":
            jdx, jdy = np.full_like(jdx, 16), np.full_like(jdy, 16)
        ntaps = 1                                                        # the reference returns before the AA pass
        key_y = sites[:, 5]
    else:
        yy, xx = np.meshgrid(rows, np.arange(W), indexing="ij")
        sx, sy = xx.ravel(), yy.ravel()
        jdx = jdy = np.ones(len(sx), dtype=np.int64)
        ntaps = {TAPS_1: 1, TAPS_REF5: 5, TAPS_4: 4}[opts.taps]
        key_y, kx = sy, sx
        if mut == "rng_pixel_from_local_row":
            key_y = np.repeat(np.arange(len(rows)), W)
    S = len(sx)
    pixel = key_y.astype(U64) * U64(W) + kx.astype(U64)
    kernel = list(AA_KERNEL)
    if mut == "taps_two_and_three_swapped":
        kernel[2], kernel[3] = kernel[3], kernel[2]
    stereo = frame.stereo_separation != 0
    eyes = (LEFT, RIGHT) if stereo else (NONE,)
    ns = frame.num_samples if frame.dof else 1
    # rays, in the order [tap][lens sample][eye][site]
    origs, dirs, draws = [], [], []
    for tap in range(ntaps):
        x = sx.astype(F64) + F64(kernel[tap][0])
        y = sy.astype(F64) + F64(kernel[tap][1])
        key = rng_key(seed, pixel, np.full(S, tap, dtype=U32)) if frame.dof else None
        for i in range(ns):
            dim = 0
            jitter = None
            for e, eye in enumerate(eyes):
                if not frame.dof:
                    o, d = screen_ray(frame, x, y, eye, None, mut)
                else:
                    u = [rng_uniform(key, np.full(S, i, dtype=U32), np.full(S, dim + k, dtype=U32)) for k in range(4)]
                    if mut == "eyes_share_one_jitter":
                        if e == 0:
                            jitter = (u[0], u[1])
                            lens = (u[2], u[3])
                            dim += 4
                        else:
                            lens = (u[0], u[1])
                            dim += 2
                        jx, jy = jitter
                    else:
                        dim += 4
                        if mut == "draws_lens_before_jitter":
                            lens, (jx, jy) = (u[0], u[1]), (u[2], u[3])
                        else:
                            (jx, jy), lens = (u[0], u[1]), (u[2], u[3])
                    draws += [jx, jy, lens[0], lens[1]]
                    o, d = screen_ray(frame, x + jx * jdx.astype(F64), y + jy * jdy.astype(F64), eye, lens, mut)
                origs.append(o)
                dirs.append(d)
    rays = np.ascontiguousarray(np.hstack([np.vstack(origs), np.vstack(dirs)]))
    recs, trace = gr.trace(T, rays)
    segs = sr.shadow_segments(Ts, rays[:, 3:], recs)
    vis, _, vis_trace = gr.test_visibility(T, segs)
    shaded = sr.shade(Ts, rays[:, 3:], recs, vis.reshape(len(rays), -1))
    ne = len(eyes)

    with np.errstate(all="ignore"):
        rgb, lo, hi = (accumulate(c, ntaps, ns, ne, frame, mut) for c in (shaded.rgb, shaded.lo, shaded.hi))
    flagged = shaded.ambiguous.reshape(ntaps * ns * ne, S).any(axis=0)

    def paint(a):
        """site values -> the rank's rows"""
        if not opts.prepass_bucket:
            return a.reshape((len(rows), W) + a.shape[1:])
        full = np.zeros((H, W) + a.shape[1:], dtype=a.dtype)
        for k, (x0, y0, dx, dy) in enumerate(sites[:, 4:]):
            full[y0:y0 + dy, x0:x0 + dx] = a[k]                           # drawRect
        return full[rows]

    r = Rendered()
    r.rgb, r.lo, r.hi, r.ambiguous = paint(rgb), paint(lo), paint(hi), paint(flagged)
    r.wide = (r.lo.view(U32) != r.hi.view(U32)).any(axis=-1)
    r.rays, r.recs, r.trace, r.vis_trace = rays, recs, trace, vis_trace
    r.draws = np.concatenate(draws) if draws else np.zeros(0)
    r.sample_ambiguous = float(shaded.ambiguous.mean())
    r.samples_per_pixel = ntaps * ns * ne
    return r


def compare(got, ref):
    """a frame against a Rendered -> (floats that differ in pixels held to their bits, floats outside [lo, hi] in the
    others); every pixel is in one of the two groups"""
    flat = sr.Shaded()
    loose = (ref.ambiguous | ref.wide).ravel()
    flat.rgb, flat.lo, flat.hi, flat.ambiguous = ref.rgb.reshape(-1, 3), ref.lo.reshape(-1, 3), ref.hi.reshape(-1, 3), loose
    got = np.ascontiguousarray(got, dtype=F32)
    assert got.size == flat.rgb.size, (got.shape, ref.rgb.shape)
    return sr.compare(got, flat)

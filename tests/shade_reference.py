"""A typed restatement of the reference's SHADING stage, independent of oracle/c2rt_oracle.c and of the device code.

Written from the reference's D source (paths relative to its source/rt/): shader.d:67-105 (Lambert.shade),
shader.d:197-250 (Phong.shade), texture.d:36-54 (Checker), texture.d:77-86 (Procedure2), texture.d:116-126
(BitmapTexture), bitmap.d:48-63 (getFilteredPixel), color.d (Color arithmetic, intensity), light.d:11-14,56-65
(PointLight) and imported_types.d:62-73 (reflect, faceforward).  gfm:math's vec3d is not part of the reference's tree;
its published algorithms are used: dot and squaredMagnitude are `sum = 0; sum += a_i * b_i`, normalize is
`v *= 1 / sqrt(squaredMagnitude)`.

Inputs are the scene descriptor's tables, ray directions, HIT RECORDS (closest_node, p, normal, u, v: geometry is an
input here, not under test) and a per-ray, per-light VISIBILITY array (Scene.testVisibility's answers for
p + N * 1e-6 -> lightPos).  Output: (n, 3) float32.

Rules of evaluation:
  - every operation in the type the D source gives it: Vector arithmetic, normalize, dot, cosTheta, cosGamma are
    np.float64; Color arithmetic is np.float32; `Color * double` / `Color / double` narrow the double first
    (color.d:128-138 take a float);
  - source order, no fused operation (numpy never contracts);
  - lights in list order, a light whose intensity(color) == 0 is skipped, `/ numSamples` is `/ 1` (light.d:56-59);
  - a miss (closest_node < 0) is the environment's black, as c2rt_trace_rays documents;
  - `^^` (pow) and sin are evaluated with mpmath at 50 digits, rounded ONCE to double and then cast to float32.
    A sample is AMBIGUOUS when one of its libm values, taken exactly, lies within 4 fp64 ulp of a float32 rounding
    midpoint (only there can a faithful, not correctly rounded libm — pow within 1 ulp, sin within 2 — cast to the
    neighbouring float), or when a sine's exact value is below 2^-100 in magnitude.  `shade` returns, for such
    samples, the per-channel range over every choice of those casts.
"""
import ctypes as C
import itertools

import mpmath
import numpy as np

F32, F64 = np.float32, np.float64
SHADER_LAMBERT, SHADER_PHONG = 0, 1
TEX_CHECKER, TEX_PROCEDURE2, TEX_BITMAP = 0, 1, 2
AMBIGUOUS_ULPS = 4

# the named misreadings of test_shade_reference's mutation check (each changes ONE statement below)
MUTATIONS = ("strength_ignored", "strength_on_lambert", "specular_times_diffuse", "lightdir_in_float", "weights_transposed",
             "no_column_wrap", "scaling_in_float", "sin_in_float", "uv_colors_swapped", "dark_light_shifts_visibility",
             "light_32_dropped")


class Tables:
    """numpy copies of the descriptor fields the shading stage reads (include/c2rt.h)"""

    def __init__(self, desc):
        d = desc.contents if hasattr(desc, "contents") else desc

        def arr(p, n, dt):
            return np.array([p[i] for i in range(n)], dtype=dt) if n else np.zeros(0, dtype=dt)
        nt, ns, nl, nn = d.n_textures, d.n_shaders, d.n_lights, d.n_nodes
        self.node_shader = arr(d.node_shader, nn, np.int64)
        self.shader_type = arr(d.shader_type, ns, np.int64)
        self.shader_color = arr(d.shader_color, 3 * ns, F32).reshape(ns, 3)
        self.shader_texture = arr(d.shader_texture, ns, np.int64)
        self.shader_exponent = arr(d.shader_exponent, ns, F64)
        self.shader_strength = arr(d.shader_strength, ns, F32)
        self.tex_type = arr(d.tex_type, nt, np.int64)
        self.tex_color = arr(d.tex_color, 18 * nt, F32).reshape(nt, 6, 3)
        self.tex_param = arr(d.tex_param, 6 * nt, F64).reshape(nt, 6)
        self.tex_scaling = arr(d.tex_scaling, nt, F32)
        self.tex_width = arr(d.tex_width, nt, np.int64)
        self.tex_height = arr(d.tex_height, nt, np.int64)
        self.tex_offset = arr(d.tex_offset, nt, np.int64)
        n_tx = int(d.n_texels)
        self.texels = (np.ctypeslib.as_array(C.cast(d.texels, C.POINTER(C.c_float)), shape=(3 * n_tx,)).astype(F32).reshape(n_tx, 3)
                       if n_tx else np.zeros((0, 3), F32))
        self.light_pos = arr(d.light_pos, 3 * nl, F64).reshape(nl, 3)
        self.light_color = arr(d.light_color, 3 * nl, F32).reshape(nl, 3)
        self.light_power = arr(d.light_power, nl, F32)
        self.ambient = np.array(list(d.ambient), dtype=F32)
        self.n_lights, self.n_nodes = nl, nn

    def light_colors(self):
        """Light.color(): lightColor * lightPower, in float — light.d:11-14"""
        return (self.light_color * self.light_power[:, None]).astype(F32)

    def lit(self):
        """lightColor.intensity() != 0 — shader.d:88,219; intensity = (r + g + b) / 3 in float, color.d:141-144"""
        c = self.light_colors()
        with np.errstate(over="ignore", invalid="ignore"):
            return ((c[:, 0] + c[:, 1]) + c[:, 2]) / F32(3) != 0


# ---- libm: mpmath at 50 digits, rounded once to double, then cast to float32 ----------------------------------------

_MP = mpmath.mp.clone()
_MP.dps = 50
_libm_cache = {}


def _to_double(x):
    """round to nearest double (float(mpf) truncates)"""
    return mpmath.libmp.to_float(x._mpf_, rnd=mpmath.libmp.round_nearest)


def _f32_midpoint_neighbour(exact, d):
    """(float32(d), other): `other` is the float32 on the far side of a rounding midpoint that `exact` lies within
    AMBIGUOUS_ULPS fp64 ulp of, or None"""
    with np.errstate(over="ignore"):
        f = F32(d)
    if not np.isfinite(f) or not np.isfinite(d):
        return f, None
    ulp = _MP.mpf(float(np.spacing(abs(F64(d)))))
    for other in (np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf))):
        if not np.isfinite(other):
            continue
        mid = (_MP.mpf(float(f)) + _MP.mpf(float(other))) / 2
        if abs(exact - mid) <= AMBIGUOUS_ULPS * ulp:
            return f, F32(other)
    return f, None


def _libm(kind, x, e=0.0):
    key = (kind, float(x), float(e))
    r = _libm_cache.get(key)
    if r is None:
        if kind == "sin":
            exact = _MP.sin(_MP.mpf(float(x)))
            f, other = _f32_midpoint_neighbour(exact, _to_double(exact))
            tiny = bool(abs(exact) < _MP.mpf(2) ** -100)      # flagged; there is no other cast to try
        else:
            exact = _MP.power(_MP.mpf(float(x)), _MP.mpf(float(e)))
            f, other = _f32_midpoint_neighbour(exact, _to_double(exact))
            tiny = False
        r = _libm_cache[key] = (f, other, tiny)
    return r


class Libm:
    """sin / pow over arrays; counts per row the values near a float32 midpoint (`ambiguous`) and the sines below
    2^-100 (`tiny`).  `flips`: the ordinals (in call order) of the near-midpoint values whose cast goes to the
    neighbour — used on ONE row at a time to bound that sample.  `note` collects named per-row flags (which branch a
    sample took), for the tests' coverage conditions."""

    def __init__(self, n, flips=()):
        self.ambiguous = np.zeros(n, dtype=np.int64)
        self.tiny = np.zeros(n, dtype=np.int64)
        self.flags = {}
        self.n = n
        self.flips = set(flips)
        self.seen = 0
        self.calls = 0

    def _apply(self, kind, rows, x, e):
        out = np.empty(len(rows), dtype=F32)
        for k, (i, xv) in enumerate(zip(rows, x)):
            f, other, tiny = _libm(kind, xv, e)
            self.tiny[i] += tiny
            if other is not None:
                self.ambiguous[i] += 1
                if self.seen in self.flips:
                    f = other
                self.seen += 1
            out[k] = f
        self.calls += len(rows)
        return out

    def sin(self, rows, x):
        return self._apply("sin", rows, x, 0.0)

    def pow(self, rows, x, e):
        return self._apply("pow", rows, x, e)

    def note(self, name, rows, mask=True):
        f = self.flags.setdefault(name, np.zeros(self.n, dtype=bool))
        f[np.asarray(rows)[np.broadcast_to(mask, np.shape(rows))]] = True


# ---- gfm:math vec3d ---------------------------------------------------------------------------------------------------


def dot(a, b):
    s = np.zeros(a.shape[:-1], dtype=F64)
    for i in range(3):
        s = s + a[..., i] * b[..., i]
    return s


def normalized(v):
    inv = F64(1) / np.sqrt(dot(v, v))
    return v * inv[..., None]


def faceforward(ray_dir, normal):
    """imported_types.d:69-73"""
    return np.where((dot(ray_dir, normal) < 0)[..., None], normal, -normal)


def reflect(ray, norm):
    """imported_types.d:62-67: ray - 2 * dot(ray, norm) * norm, normalised"""
    return normalized(ray - (F64(2) * dot(ray, norm))[..., None] * norm)


# ---- textures ---------------------------------------------------------------------------------------------------------


def _x86_cast_int(x):
    """D's cast(int) of a double on x86-64 (cvttsd2si): truncation; the `integer indefinite` 0x80000000 for NaN and
    for values outside int's range"""
    with np.errstate(invalid="ignore"):
        t = np.trunc(x)
        ok = np.isfinite(t) & (t >= -2147483648.0) & (t <= 2147483647.0)
        return np.where(ok, np.where(ok, t, 0).astype(np.int64), np.int64(-2147483648))


def _checker(T, t, u, v, rows, libm):
    """texture.d:48-53"""
    size = T.tex_param[t, 0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = _x86_cast_int(np.floor(u / size))
        y = _x86_cast_int(np.floor(v / size))
    s = (x + y + 2147483648) % 4294967296 - 2147483648          # int + int wraps
    white = np.fmod(s, 2)                                        # D's %: the sign of the dividend
    libm.note("checker_color1", rows, white == 0)
    libm.note("checker_color2", rows, white != 0)
    return np.where((white != 0)[:, None], T.tex_color[t, 1], T.tex_color[t, 0]).astype(F32)


def _procedure2(T, t, u, v, rows, libm, mut):
    """texture.d:79-85: result += colorU[i] * sin(u * freqU[i]) + colorV[i] * sin(v * freqV[i])"""
    cu, cv = T.tex_color[t, 0:3], T.tex_color[t, 3:6]
    if mut == "uv_colors_swapped":
        cu, cv = cv, cu
    result = np.zeros((len(u), 3), dtype=F32)
    for i in range(3):
        au, av = u * T.tex_param[t, i], v * T.tex_param[t, 3 + i]
        if mut == "sin_in_float":
            su, sv = np.sin(au.astype(F32)), np.sin(av.astype(F32))
        else:
            su, sv = libm.sin(rows, au), libm.sin(rows, av)
        result = result + (cu[i][None, :] * su[:, None] + cv[i][None, :] * sv[:, None])
    return result


def _bitmap(T, t, u, v, rows, libm, mut):
    """texture.d:118-125 and bitmap.d:50-62"""
    w, h, off = int(T.tex_width[t]), int(T.tex_height[t]), int(T.tex_offset[t])
    sc = T.tex_scaling[t]
    with np.errstate(invalid="ignore", over="ignore"):
        if mut == "scaling_in_float":
            u, v = (u.astype(F32) * sc).astype(F64), (v.astype(F32) * sc).astype(F64)
        else:
            u, v = u * F64(sc), v * F64(sc)
        u, v = u - np.floor(u), v - np.floor(v)
        x, y = u.astype(F32) * F32(w), v.astype(F32) * F32(h)       # cast(float) u * bmp.width: a float product
        invalid = ~((x < F32(w)) & (y < F32(h)))                    # isInvalidPos(cast(size_t) x, cast(size_t) y); NaN too
        xs, ys = np.where(invalid, F32(0), x), np.where(invalid, F32(0), y)
        tx, ty = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
        tx_next, ty_next = (tx + 1) % w, (ty + 1) % h
        p, q = xs - tx.astype(F32), ys - ty.astype(F32)
        one = F32(1)
        w00, w10, w01, w11 = (one - p) * (one - q), p * (one - q), (one - p) * q, p * q
        if mut == "weights_transposed":
            w10, w01 = w01, w10

        def px(cx, cy):
            idx = off + cy * w + cx
            return T.texels[np.minimum(idx, len(T.texels) - 1)]
        libm.note("bitmap_red", rows, invalid)
        libm.note("bitmap_wrapped_column", rows, ~invalid & (tx == w - 1))
        libm.note("bitmap_wrapped_row", rows, ~invalid & (ty == h - 1))
        nx = tx + 1 if mut == "no_column_wrap" else tx_next
        col = ((px(tx, ty) * w00[:, None] + px(nx, ty) * w10[:, None]) + px(tx, ty_next) * w01[:, None]) + px(nx, ty_next) * w11[:, None]
    return np.where(invalid[:, None], np.array([1, 0, 0], dtype=F32), col).astype(F32)


def tex_color(T, t, u, v, libm=None, mut=None):
    """Texture.getTexColor of texture `t` at (u, v) arrays: (n, 3) float32.  With libm=None returns (colour, ambiguous)."""
    u, v = np.asarray(u, dtype=F64), np.asarray(v, dtype=F64)
    own = libm is None
    if own:
        libm = Libm(len(u))
    rows = np.arange(len(u))
    kind = T.tex_type[t]
    if kind == TEX_CHECKER:
        c = _checker(T, t, u, v, rows, libm)
    elif kind == TEX_PROCEDURE2:
        c = _procedure2(T, t, u, v, rows, libm, mut)
    else:
        c = _bitmap(T, t, u, v, rows, libm, mut)
    return (c, (libm.ambiguous > 0) | (libm.tiny > 0)) if own else c


# ---- shade --------------------------------------------------------------------------------------------------------------


def evaluate(T, dirs, recs, vis, libm, mut=None):
    """Lambert.shade / Phong.shade (shader.d:67-105, 197-250) of every record; `libm` supplies sin and pow"""
    n = len(recs)
    out = np.zeros((n, 3), dtype=F32)
    hit = np.nonzero(recs["closest_node"] >= 0)[0]
    if not len(hit):
        return out
    rd = np.asarray(dirs, dtype=F64)[hit]
    p, nrm = recs["p"][hit], recs["normal"][hit]
    sh = T.node_shader[recs["closest_node"][hit]]
    phong = T.shader_type[sh] == SHADER_PHONG
    N = faceforward(rd, nrm)                                                        # shader.d:70,200
    diffuse = T.shader_color[sh].copy()                                             # shader.d:74-76,202-203
    tex = T.shader_texture[sh]
    for t in np.unique(tex[tex >= 0]):
        m = np.nonzero(tex == t)[0]
        sub = _SubLibm(libm, hit[m])
        diffuse[m] = tex_color(T, int(t), recs["u"][hit][m], recs["v"][hit][m], sub, mut)
    lightContrib = np.broadcast_to(T.ambient, (len(hit), 3)).astype(F32)            # shader.d:78,205
    specular = np.zeros((len(hit), 3), dtype=F32)
    colors, lit = T.light_colors(), T.lit()
    exponent, strength = T.shader_exponent[sh], T.shader_strength[sh]
    vis = np.asarray(vis).reshape(n, -1)[hit].astype(bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for l in range(T.n_lights):
            if mut == "light_32_dropped" and l == 32:
                continue
            if not lit[l]:                                                          # intensity() != 0 && ... : no shadow test
                continue
            v_l = vis[:, l - 1] if (mut == "dark_light_shifts_visibility" and l > 0 and not lit[l - 1]) else vis[:, l]
            a = np.nonzero(v_l)[0]
            if not len(a):
                continue
            lightPos = T.light_pos[l]
            if mut == "lightdir_in_float":
                ld32 = (lightPos - p[a]).astype(F32)
                s32 = np.zeros(len(a), dtype=F32)
                for i in range(3):
                    s32 = s32 + ld32[:, i] * ld32[:, i]
                lightDir = (ld32 * (F32(1) / np.sqrt(s32))[:, None]).astype(F64)
            else:
                lightDir = normalized(lightPos - p[a])                              # shader.d:90-91,221-222
            cosTheta = dot(lightDir, N[a])                                          # :95,226
            libm.note("costheta_le0_visible", hit[a], ~(cosTheta > 0))
            d = p[a] - lightPos
            baseLight = colors[l][None, :] / dot(d, d).astype(F32)[:, None]         # :98,229  Color / float(double)
            lam = baseLight * cosTheta.astype(F32)[:, None]                         # :98,231  Color * float(double)
            if mut == "strength_on_lambert":
                lam = np.where(phong[a][:, None], lam * strength[a][:, None], lam)
            avgColor = np.where((cosTheta > 0)[:, None], np.zeros(3, F32) + lam, np.zeros(3, F32)).astype(F32)
            lightContrib[a] = lightContrib[a] + avgColor                            # :102,243 (/ 1)
            ph = np.nonzero(phong[a])[0]
            if len(ph):
                R = reflect(-lightDir[ph], N[a][ph])                                # :235
                cosGamma = dot(R, -rd[a][ph])                                       # :237
                g = np.nonzero(cosGamma > 0)[0]                                     # :238
                libm.note("cosgamma_gt0", hit[a[ph]], cosGamma > 0)
                libm.note("cosgamma_le0", hit[a[ph]], ~(cosGamma > 0))
                if len(g):
                    rows = a[ph][g]
                    spec = np.zeros((len(g), 3), dtype=F32)
                    for e in np.unique(exponent[rows]):
                        k = np.nonzero(exponent[rows] == e)[0]
                        pw = libm.pow(hit[rows[k]], cosGamma[g][k], e)              # cosGamma ^^ exponent, then float
                        s = baseLight[ph][g][k] * pw[:, None]
                        if mut not in ("strength_ignored", "strength_on_lambert"):
                            s = s * strength[rows[k]][:, None]                      # :239
                        spec[k] = s
                    specular[rows] = specular[rows] + (np.zeros(3, F32) + spec)     # :244
    res = diffuse * lightContrib                                                    # :104,249
    if mut == "specular_times_diffuse":
        res = np.where(phong[:, None], diffuse * (lightContrib + specular), res)
    else:
        res = np.where(phong[:, None], res + specular, res)
    out[hit] = res
    return out


class _SubLibm:
    """maps the row numbers of a subset back to the caller's"""

    def __init__(self, libm, index):
        self.libm, self.index = libm, index

    def sin(self, rows, x):
        return self.libm.sin(self.index[rows], x)

    def pow(self, rows, x, e):
        return self.libm.pow(self.index[rows], x, e)

    def note(self, name, rows, mask=True):
        self.libm.note(name, self.index[rows], mask)


MAX_AMBIGUOUS_PER_SAMPLE = 8


class Shaded:
    """rgb (n, 3) float32 | ambiguous (n,) bool: near a midpoint or a tiny sine | lo, hi: per-channel bounds over every
    choice of the near-midpoint casts (equal to rgb elsewhere) | midpoint, tiny: the two reasons | flags: name -> (n,)
    bool, the branches each sample took | libm_calls"""


def shade(T, dirs, recs, vis, mut=None):
    """-> Shaded"""
    n = len(recs)
    dirs = np.asarray(dirs, dtype=F64)
    vis = np.asarray(vis).reshape(n, -1)
    libm = Libm(n)
    rgb = evaluate(T, dirs, recs, vis, libm, mut)
    lo, hi = rgb.copy(), rgb.copy()
    for i in np.nonzero(libm.ambiguous)[0]:
        k = int(libm.ambiguous[i])
        assert k <= MAX_AMBIGUOUS_PER_SAMPLE, (i, k)
        for r in range(1, k + 1):
            for flips in itertools.combinations(range(k), r):
                alt = evaluate(T, dirs[i:i + 1], recs[i:i + 1], vis[i:i + 1], Libm(1, flips), mut)[0]
                with np.errstate(invalid="ignore"):
                    lo[i], hi[i] = np.fmin(lo[i], alt), np.fmax(hi[i], alt)
    r = Shaded()
    r.rgb, r.lo, r.hi = rgb, lo, hi
    r.midpoint, r.tiny = libm.ambiguous > 0, libm.tiny > 0
    r.ambiguous = r.midpoint | r.tiny
    r.flags, r.libm_calls = libm.flags, libm.calls
    return r


def facing_normals(dirs, recs):
    """N of every record (faceforward), for the shadow segments p + N * 1e-6 -> lightPos (shader.d:88,219)"""
    return faceforward(np.asarray(dirs, dtype=F64), recs["normal"])


def shadow_segments(T, dirs, recs):
    """(n * n_lights, 6): from p + N * 1e-6 to every light, ray-major; rows of misses hold zeros"""
    N = facing_normals(dirs, recs)
    frm = np.where((recs["closest_node"] >= 0)[:, None], recs["p"] + N * 1e-6, 0.0)
    n, nl = len(recs), T.n_lights
    seg = np.empty((n, nl, 6), dtype=F64)
    seg[:, :, :3] = frm[:, None, :]
    seg[:, :, 3:] = T.light_pos[None, :, :]
    return seg.reshape(n * nl, 6)


def compare(got, ref):
    """got against a Shaded -> (differing floats outside ambiguous samples, floats of ambiguous samples outside their bounds), comparing
    BITS (so -0 != +0) outside the ambiguous samples, NaN equal to NaN"""
    got = np.ascontiguousarray(got, dtype=F32).reshape(-1, 3)
    rgb, ambiguous, lo, hi = ref.rgb, ref.ambiguous, ref.lo, ref.hi
    same = (got.view(np.uint32) == np.ascontiguousarray(rgb).view(np.uint32)) | (np.isnan(got) & np.isnan(rgb))
    plain = int((~same[~ambiguous]).sum())
    with np.errstate(invalid="ignore"):
        inside = (got >= lo) & (got <= hi) | (np.isnan(got) & np.isnan(rgb))
    return plain, int((~inside[ambiguous]).sum())

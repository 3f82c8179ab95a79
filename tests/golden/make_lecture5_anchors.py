#!/usr/bin/env python3
"""Independent anchors for the headline scene, lecture5.sdl: Sphere, Cube, CsgOp / CsgDiff, Node translate, Phong,
Lambert + bitmap (8- and 24-bpp), testVisibility and the 5-tap antialiasing.

Writes tests/golden/lecture5_anchors.json.  NOT reference output and NOT produced by the oracle, the host mirror or
the kernels: new Python over mpmath's `mpf`, written from the algorithm of the reference with the cited lines open
beside it.  The rules of make_zaphod_anchors.py hold here too:

  * nothing is imported from oracle/, chess2rt_amd/ or tests/, and no file of theirs is read.  The only files read
    are tests/golden/scenes/floor.bmp and world.bmp, through the BMP reader below (imageio/bmp.d:60-193: 24-bpp and
    8-bpp palette, rows stored bottom-up).  The scene constants are typed in from lecture5.sdl.
  * mp.dps = 50.  Every branch (closest node, leaf, root, face, CSG walk, normal flip, light visibility) is decided
    here, and the category expected of every pixel is ASSERTED: a pixel that drifts into another category fails in
    this script, not in a test.

What is followed (file:line of the reference)
---------------------------------------------
rt/camera.d:77-147      beginFrame and getScreenRay.  lecture5 has yaw = roll = 0, so the closed form of the zaphod
                        script reduces to v * Rx(pitch) = (a, b cp + c sp, -b sp + c cp) for v = (a, b, c).
rt/renderer.d:325-376   trace: nodes in file order, data.dist = 1e99, no environment: the background is (0, 0, 0).
rt/node.d:24-47         Node.intersect: origin minus the offset (the matrices are the identity), dist times / over
                        |dir|, the direction renormalised, the point plus the offset.
rt/geometry.d:30-59     Plane (limit is never set by deserialize: NaN, every comparison with it is false).
rt/geometry.d:92-125    Sphere: sol = x2, x1 if x2 < 0; sol > dist rejects; u = (PI + atan2(dz, dx)) / (2 PI),
                        v = 1 - (PI/2 + asin(dy / R)) / PI.
rt/geometry.d:172-235   Cube: the Y pair, then the X pair through project(., 1, 0, 2) and the Z pair through
                        project(., 0, 2, 1) (rt/imported_types.d:44-60); u, v are taken in the PROJECTED frame:
                        Y faces (x - cx, z - cz), X faces (y - cy, z - cz), Z faces (x - cx, y - cy).
rt/geometry.d:271-332   findAllIntersections restarts from p + dir * 1e-6 and adds the lengths of the legs WITHOUT the
                        1e-6 steps: the k-th hit's dist is k-1 micro-units short of |p - orig|.  The walk sorts by
                        dist (rt/intersectable.d:27-32), starts from the parities, returns the first boolOp hit.
rt/geometry.d:382-397   CsgDiff flips the normal where right.isInside(p - 1e-6 dir) != right.isInside(p + 1e-6 dir).
rt/shader.d:67-105      Lambert.shade; rt/shader.d:197-250 Phong.shade; reflect and faceforward rt/imported_types.d:62-73.
rt/scene.d:62-78        testVisibility: from p + N * 1e-6, dist = |to - from|, the first node that hits blocks.
rt/light.d:8-14,52-66   PointLight: colour * power, one sample.
rt/texture.d:117-128    BitmapTexture.getTexColor; rt/bitmap.d:48-63 getFilteredPixel; rt/bitmap.d:116-126 sRGB;
                        rt/texture.d:137-138 assumedGamma 2.2 (the default) selects the sRGB branch.
rt/color.d:60-66        Color(uint): byte * (1.0f / 255.0f).
rt/renderer.d:233-251   renderPixelAA: taps (0,0) (.3,.3) (.6,0) (0,.6) (.6,.6), accumulated and divided by 5.

fp32 in the reference, and the colour tolerance
-----------------------------------------------
`Color` holds floats.  Two kinds of narrowing are told apart here.
(a) Values whose ABSOLUTE position matters are narrowed here exactly as there, with one round-to-nearest to 24 bits:
    the float constants (scaling 0.005f, ambient 0.2f, the shader colours, 1.0f/255.0f, the sRGB literals), and in
    getTexColor `cast(float) u`, the products tx = float(u) * width and ty, and p = x - tx, q = y - ty (exact in
    fp32).  The generator asserts that no such value lies within 1e-6 ulp of a rounding boundary.
(b) Roundings of a non-negative colour channel, each at most 2^-24 relative.  Counted per channel path:
    Lambert + bitmap, K = 20:  byte * divider 1; sRGB: + 0.055f, / 1.055f, ^^ 2.4f 3 (rt/bitmap.d:121-124);
      bilinear weights 1 - p, 1 - q, product 3; texel * weight 1; the three sums 3 (rt/bitmap.d:59-62);
      lightColor * lightPower 1 (rt/light.d:12); squaredMagnitude to float and the division 2, cosTheta to float and
      the product 2 (rt/shader.d:98); avgColor / numSamples 1 (:102); lightContrib += 1 (:102); diffuse *
      lightContrib 1 (:104).  The texel path of K is 11, the light path 9.
    Phong, K = 9:  baseLight 3 (rt/shader.d:229, rt/light.d:12); then either cosTheta to float and product 2 (:231),
      / numSamples 1, lightContrib += 1 (:243), diffuse * lightContrib 1 (:249); or the power to float and product 2,
      * strength 1 (:239), / numSamples 1, specular += 1 (:244); and the closing sum 1 (:249): 3 + 5 + 1.
    All terms are non-negative, nothing cancels, so a channel is off by at most K * 2^-24 * value to first order; the
    tolerance is 2 K * (2^-24 * value + 2^-149) (the second term: a specular term of 1e-100 is a zero or a subnormal in
    fp32, where a rounding is absolute: 2^-149) PLUS the geometry tolerances pushed through the channel (|rgb(x + tol_x) -
    rgb(x)| summed over dir, p, normal, u, v, each evaluated here in 50 digits).  Condition: <= 5e-6 * max(1, value).
    5-tap mean: sum of the tap tolerances / 5 plus 6 roundings of the mean (4 additions, the division, the store).

Geometry tolerance: every pixel is evaluated a second time with mp.prec = 53 (each + - * / sqrt rounded as
binary64).  tol = max(16 |value53 - value50|, 8 ulp of the largest magnitude entering the quantity); it must not
exceed 1e-9 for t, p and the lengths u, v of planes and cubes, nor 1e-12 for dir, normal and the spheres' u, v.

Robustness.  Every decision is recorded with the quantity q it tests and the magnitude s of what enters q:
  * |q| / s >= 1e-6 (s = 1e3 for distances and points: the scene's scale; s = 1 for cosines), or
  * the decision is one the ALGORITHM makes 1e-6 away from a surface on purpose (restarts of findAllIntersections,
    the two isInside probes, shadow rays leaving p + N * 1e-6): |q| is of order 1e-6 * cos(incidence) by
    construction and cannot be 1e-6 of the scene; there |q| >= 1e-7 is required, a million times the binary64
    rounding of a coordinate of this scene (1e3 * 2^-53 = 1.1e-13).
  * bilinear p, q at least 1e-6 from 0 and 1.

Misreadings.  For each named single misreading the pixels it applies to are evaluated again; the ratio is the
largest |misread - anchor| / tolerance over rgb, t, p, normal, u, v of a pixel, and the JSON stores the smallest
ratio over those pixels.  The tests require 100.  A misreading that lecture5 cannot show is listed under
`not_constrained` with the reason.

Usage: python tests/golden/make_lecture5_anchors.py   (needs mpmath; the committed JSON is what the tests read)
"""
import json
import os
import struct
import sys

from mpmath import mp, mpf, sqrt, atan2, asin, floor, tan, cos, sin, pi, workprec

mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 640, 480
BIG = mpf("1e99")
TAPS = ((0, 0), ("0.3", "0.3"), ("0.6", 0), (0, "0.6"), ("0.6", "0.6"))          # rt/renderer.d:235-242
K_LAMBERT_BITMAP, K_PHONG, K_AA = 20, 9, 6
EPS24 = mpf(2) ** -24


def f32(x):
    """round to nearest fp32 (one rounding, ties to even; nothing here is subnormal)"""
    with workprec(24):
        return +mpf(x)


def dbl(text):
    """a decimal of the scene file as the binary64 the reference's parser holds"""
    return mpf(float(text))


def add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def scl(a, s):
    return tuple(x * s for x in a)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def norm(a):
    return sqrt(dot(a, a))


def unit(a):
    return scl(a, 1 / norm(a))


def neg(a):
    return (-a[0], -a[1], -a[2])


# ---- the two textures, imageio/bmp.d:60-193 ---------------------------------------------------------------------------
def read_bmp(name):
    """-> (width, height, rows) with rows[y][x] = (r, g, b) bytes and y = 0 the TOP row: the file stores the bottom row
    first (foreach_reverse over y, imageio/bmp.d:150,170)."""
    b = open(os.path.join(HERE, "scenes", name), "rb").read()
    assert b[:2] == b"BM"
    pix_off = struct.unpack_from("<I", b, 10)[0]
    hdr, w, h, planes, bpp, compression = struct.unpack_from("<IiiHHI", b, 14)
    colors_used = struct.unpack_from("<I", b, 14 + 32)[0]
    assert hdr == 40 and planes == 1 and compression == 0 and h > 0 and bpp in (8, 24)
    rows = [None] * h
    if bpp == 24:
        stride = (24 * w + 31) // 32 * 4                 # rows are padded to four bytes
        for k in range(h):                               # k-th stored row is image row h - 1 - k
            o = pix_off + k * stride
            rows[h - 1 - k] = [(b[o + 3 * x + 2], b[o + 3 * x + 1], b[o + 3 * x]) for x in range(w)]
    else:
        pal = [struct.unpack_from("<BBBB", b, 14 + hdr + 4 * i) for i in range(colors_used or 256)]     # B, G, R, 0
        assert w % 4 == 0                                # the 8-bpp branch reads `width` bytes a row, no padding skipped
        for k in range(h):
            o = pix_off + k * w
            rows[h - 1 - k] = [(pal[i][2], pal[i][1], pal[i][0]) for i in b[o:o + w]]
    return w, h, rows


BITMAPS = {"floor.bmp": read_bmp("floor.bmp"), "world.bmp": read_bmp("world.bmp")}


class Margins:
    """the robustness conditions of the docstring; `worst` keeps the smallest margin of each kind for the JSON"""

    def __init__(self):
        self.worst = {"far": mpf(1), "offset": mpf(1), "texel": mpf(1), "fp32": mpf(1)}
        self.fail = None

    def _note(self, kind, m, what):
        if m < self.worst[kind]:
            self.worst[kind] = m
        lim = {"far": mpf("1e-6"), "offset": mpf("1e-7"), "texel": mpf("1e-6"), "fp32": mpf("1e-6")}[kind]
        if m < lim and self.fail is None:
            self.fail = "%s margin %s of %s" % (kind, mp.nstr(m, 5), what)

    def decide(self, q, s, what, offset_ray=False):
        """records the decision `q <> 0` (q of magnitude-scale s) and returns q"""
        if abs(q) >= mpf("1e-6") * s:
            self._note("far", abs(q) / s, what)
        elif offset_ray:
            self._note("offset", abs(q), what)
        else:
            self._note("far", abs(q) / s, what)
        return q

    def texel(self, p, what):
        self._note("texel", min(p, 1 - p), what)

    def narrowed(self, x, what):
        y = f32(x)
        if x != 0:
            ulp = mpf(2) ** (floor(mp.log(abs(y), 2)) - 23)
            self._note("fp32", mpf("0.5") - abs(x - y) / ulp, what)
        return y


L = mpf(1000)                                            # the scene's scale: coordinates of 1e2 .. 1e3


class Scene:
    """lecture5.sdl, typed in; built at the precision in force so that the 53-bit pass holds 53-bit constants"""

    def __init__(self, mis=()):
        self.mis = frozenset(mis)
        self.cam_pos = (mpf(0), mpf(165), mpf(0))
        self.pitch, self.fov = mpf(-30), mpf(90)
        self.light_pos = (mpf(-90), mpf(700), mpf(350))
        self.light_color, self.light_power = (mpf(1), mpf(1), mpf(1)), mpf(800000)
        self.ambient = (f32(dbl("0.2")),) * 3
        self.geoms = {
            "floor": ("plane", dbl("-0.01")),
            "globe_ball": ("sphere", (mpf(100), mpf(50), mpf(320)), mpf(50)),
            "cube": ("cube", (mpf(-100), mpf(60), mpf(200)), mpf(100)),
            "sphere": ("sphere", (mpf(-100), mpf(60), mpf(200)), mpf(70)),
            "diff": ("diff", "cube", "sphere"),
            "S": ("sphere", (mpf(0), mpf(0), mpf(0)), mpf(15)),
        }
        self.textures = {"bmp": ("floor.bmp", f32(dbl("0.005"))), "world": ("world.bmp", mpf(1))}
        ex = {"exp79": -1, "exp81": 1}
        de = sum(v for k, v in ex.items() if k in self.mis)
        self.shaders = {
            "floor_shader": ("lambert", "bmp"),
            "globe_shader": ("lambert", "world"),
            "csg_shader": ("phong", (f32(dbl("0.5")), f32(dbl("0.5")), mpf(0)), mpf(60 + de), mpf(1)),
            "ball_shader": ("phong", (mpf(0), mpf(0), f32(dbl("0.6"))), mpf(80 + de), mpf(1)),
        }
        zero = (mpf(0), mpf(0), mpf(0))
        self.nodes = [("floor", "floor", "floor_shader", zero), ("globe", "globe_ball", "globe_shader", zero),
                      ("csgNode", "diff", "csg_shader", zero),
                      ("S1", "S", "ball_shader", (mpf(100), mpf(15), mpf(256))),
                      ("S2", "S", "ball_shader", (mpf(100), mpf(15), mpf(206))),
                      ("S3", "S", "ball_shader", (mpf(100), mpf(15), mpf(156)))]
        self.e6 = dbl("1e-6")
        self.e9 = dbl("1e-9")
        # Camera.beginFrame, rt/camera.d:77-117, yaw = roll = 0
        aspect = mpf(W) / H
        scaling = tan(self.fov / 2 * pi / 180) / sqrt(aspect * aspect + 1)
        cp, sp = cos(self.pitch * pi / 180), sin(self.pitch * pi / 180)
        rot = lambda v: (v[0], v[1] * cp + v[2] * sp, -v[1] * sp + v[2] * cp)
        x, y = -aspect * scaling, scaling
        self.up_left = add(rot((x, y, 1)), self.cam_pos)
        self.up_right = add(rot((-x, y, 1)), self.cam_pos)
        self.down_left = add(rot((x, -y, 1)), self.cam_pos)
        self.right_dir, self.up_dir, self.front_dir = rot((1, 0, 0)), rot((0, 1, 0)), rot((0, 0, 1))
        assert self.front_dir[1] < 0 < self.front_dir[2]  # pitch -30 looks down at the floor

    def screen_ray(self, x, y):                          # rt/camera.d:123-147
        t = add(add(self.up_left, scl(sub(self.up_right, self.up_left), mpf(x) / W)),
                scl(sub(self.down_left, self.up_left), mpf(y) / H))
        return unit(sub(t, self.cam_pos))

    # ---- geometry: each returns a hit dict or None; `best` is data.dist on entry ----------------------------------
    def plane(self, g, o, d, best, M, off):
        y = g[1]
        M.decide(o[1] - y, L, "plane side", off)
        if o[1] > y:
            M.decide(d[1] + self.e9, mpf(1), "plane horizon")
            if d[1] > -self.e9:
                return None
        elif o[1] < y:
            M.decide(d[1] - self.e9, mpf(1), "plane horizon")
            if d[1] < self.e9:
                return None
        mult = (o[1] - y) / -d[1]
        if best < BIG:
            M.decide(mult - best, L, "plane against best", off)
        if mult > best:
            return None
        p = add(o, scl(d, mult))
        return {"p": p, "dist": mult, "normal": (mpf(0), mpf(1), mpf(0)), "u": p[0], "v": p[2], "g": "floor", "mag": L}

    def sphere(self, name, g, o, d, best, M, off):
        c, R = g[1], g[2]
        Hv = sub(o, c)
        A = dot(d, d)
        B = 2 * dot(Hv, d)
        Cc = dot(Hv, Hv) - R * R
        D = B * B - 4 * A * Cc
        M.decide(D, B * B + 4 * A * abs(Cc), "discriminant of " + name, off)
        if D < 0:
            return None
        x1 = (-B + sqrt(D)) / (2 * A)
        x2 = (-B - sqrt(D)) / (2 * A)
        if "root_swap" in self.mis:
            x1, x2 = x2, x1
        sol = x2
        M.decide(x2, L, "near root of " + name, off)
        if sol < 0:
            sol = x1
            M.decide(x1, L, "far root of " + name, off)
        if sol < 0:
            return None
        if best < BIG:
            M.decide(sol - best, L, name + " against best", off)
        if sol > best:
            return None
        p = add(o, scl(d, sol))
        n = unit(sub(p, c))
        if "sphere_u_atan2_xz" in self.mis:
            angle = atan2(p[0] - c[0], p[2] - c[2])
        else:
            angle = atan2(p[2] - c[2], p[0] - c[0])
        u = (pi + angle) / (2 * pi)
        v = (pi / 2 + asin((p[1] - c[1]) / R)) / pi
        if "sphere_v_no_one_minus" not in self.mis:
            v = 1 - v
        return {"p": p, "dist": sol, "normal": n, "u": u, "v": v, "g": name, "mag": mpf(1)}

    def cube_side(self, o, d, c, half, best, M, off):
        if abs(d[1]) < self.e9:
            return None
        M.decide(abs(d[1]) - self.e9, mpf(1), "cube side parallel")
        hit = None
        for side in (-1, 1):
            mult = (o[1] - (c[1] + side * half)) / -d[1]
            M.decide(mult, L, "cube side behind", off)
            if mult < 0:
                continue
            if best < BIG:
                M.decide(mult - best, L, "cube side against best", off)
            if mult > best:
                continue
            p = add(o, scl(d, mult))
            for q in (p[0] - (c[0] - half), (c[0] + half) - p[0], p[2] - (c[2] - half), (c[2] + half) - p[2]):
                M.decide(q, L, "cube face bounds", off)
            if p[0] < c[0] - half or p[0] > c[0] + half or p[2] < c[2] - half or p[2] > c[2] + half:
                continue
            hit = {"p": p, "dist": mult, "normal": (mpf(0), mpf(side), mpf(0)), "u": p[0] - c[0], "v": p[2] - c[2]}
            best = mult
        return hit

    def cube(self, name, g, o, d, best, M, off):
        c, half = g[1], g[2] * mpf("0.5")
        found = None
        # the identity, then the two swaps of rt/imported_types.d:44-60 (each is its own inverse)
        for perm in ((0, 1, 2), (1, 0, 2), (0, 2, 1)):
            pj = lambda v: (v[perm[0]], v[perm[1]], v[perm[2]])
            h = self.cube_side(pj(o), pj(d), pj(c), half, best, M, off)
            if h:
                h["p"], h["normal"] = pj(h["p"]), pj(h["normal"])
                if "cube_uv_unpermuted" in self.mis:
                    h["u"], h["v"] = h["p"][0] - c[0], h["p"][2] - c[2]
                found, best = h, h["dist"]
        if found:
            found["g"], found["mag"] = name, L
        return found

    def find_all(self, name, o, d, M, off):                   # rt/geometry.d:271-290
        out, cur = [], mpf(0)
        while True:
            h = self.geom(name, o, d, BIG, M, off)
            if not h:
                return out
            h["dist"] += cur
            cur = h["dist"]
            o = add(h["p"], scl(d, self.e6))
            off = True
            out.append(h)
            assert len(out) <= 4

    def inside_sphere(self, g, p, M):
        c, R = g[1], g[2]
        M.decide(norm(sub(c, p)) - R, L, "isInside probe", True)
        return dot(sub(c, p), sub(c, p)) < R * R

    def diff(self, g, o, d, best, M, off):
        left, right = g[1], g[2]
        lh, rh = self.find_all(left, o, d, M, off), self.find_all(right, o, d, M, off)
        allh = sorted(lh + rh, key=lambda h: h["dist"])
        for a, b in zip(allh, allh[1:]):
            M.decide(b["dist"] - a["dist"], L, "order of CSG hits")
        in_l, in_r = len(lh) % 2 == 1, len(rh) % 2 == 1
        hit = None
        for h in allh:
            if h["g"] == left:
                in_l = not in_l
            else:
                in_r = not in_r
            if in_l and not in_r:
                if best < BIG:
                    M.decide(h["dist"] - best, L, "CSG hit against best", off)
                if h["dist"] > best:
                    return None
                hit = dict(h)
                break
        if hit is None:
            return None
        rg = self.geoms[right]
        before = self.inside_sphere(rg, sub(hit["p"], scl(d, self.e6)), M)
        after = self.inside_sphere(rg, add(hit["p"], scl(d, self.e6)), M)
        hit["flipped"] = before != after
        if hit["flipped"] and "no_flip" not in self.mis:
            hit["normal"] = neg(hit["normal"])
        hit["csg"] = {"left_hits": len(lh), "right_hits": len(rh)}
        return hit

    def geom(self, name, o, d, best, M, off):
        g = self.geoms[name]
        if g[0] == "plane":
            return self.plane(g, o, d, best, M, off)
        if g[0] == "sphere":
            return self.sphere(name, g, o, d, best, M, off)
        if g[0] == "cube":
            return self.cube(name, g, o, d, best, M, off)
        return self.diff(g, o, d, best, M, off)

    def node_hit(self, node, o, d, best, M, off):        # rt/node.d:24-47, identity matrices
        _, gname, _, offset = node
        oc = sub(o, offset)
        length = norm(d)
        h = self.geom(gname, oc, scl(d, 1 / length), best * length if best < BIG else best, M, off)
        if not h:
            return None
        h["normal"] = unit(h["normal"])
        h["p_object"], h["dist_object"], h["orig_object"] = h["p"], h["dist"], oc
        h["p"] = add(h["p"], offset)
        h["dist"] = h["dist"] / length
        return h

    def trace(self, o, d, M):
        best, hit, closest = BIG, None, None
        for node in self.nodes:
            h = self.node_hit(node, o, d, best, M, False)
            if h:
                best, hit, closest = h["dist"], h, node
        return closest, hit

    def visible(self, frm, to, M):                       # rt/scene.d:62-78
        d = unit(sub(to, frm))
        dist = norm(sub(to, frm))
        for node in self.nodes:
            if self.node_hit(node, frm, d, dist, M, True):
                return False, node[0]
        return True, None

    # ---- textures and shaders ------------------------------------------------------------------------------------
    def srgb(self, v):                                   # rt/bitmap.d:116-126, the literals are floats
        if "no_srgb" in self.mis or v == 0 or v == 1:
            return v
        if v <= f32(dbl("0.04045")):
            return v / f32(dbl("12.92"))
        return ((v + f32(dbl("0.055"))) / f32(dbl("1.055"))) ** f32(dbl("2.4"))

    def texel(self, bmp, tx, ty):
        w, h, rows = bmp
        r, g, b = rows[h - 1 - ty if "rows_top_down" in self.mis else ty][tx]
        div = f32(mpf(1) / 255)                          # rt/color.d:62: enum divider = 1.0f / 255.0f
        return tuple(self.srgb(c * div) for c in (r, g, b))

    def tex_color(self, tname, u, v, M, info):           # rt/texture.d:117-128, rt/bitmap.d:48-63
        fname, scaling = self.textures[tname]
        bmp = BITMAPS[fname]
        w, h = bmp[0], bmp[1]
        if "scaling_divides" in self.mis:
            u, v = u / scaling, v / scaling
        else:
            u, v = u * scaling, v * scaling
        u, v = u - floor(u), v - floor(v)
        x = M.narrowed(M.narrowed(u, "float(u)") * w, "tx")
        y = M.narrowed(M.narrowed(v, "float(v)") * h, "ty")
        assert int(x) < w and int(y) < h                 # else the reference answers red (rt/bitmap.d:50-51)
        tx, ty = int(floor(x)), int(floor(y))
        p, q = x - tx, y - ty
        M.texel(p, "bilinear p")
        M.texel(q, "bilinear q")
        txn, tyn = (tx + 1) % w, (ty + 1) % h
        c00, c10, c01, c11 = self.texel(bmp, tx, ty), self.texel(bmp, txn, ty), self.texel(bmp, tx, tyn), self.texel(bmp, txn, tyn)
        info["texel"], info["bilinear_pq"] = [tx, ty], [p, q]
        return tuple(c00[k] * ((1 - p) * (1 - q)) + c10[k] * (p * (1 - q)) + c01[k] * ((1 - p) * q) + c11[k] * (p * q)
                     for k in range(3))

    def shade(self, node, d, hit, M, lit=None):
        """-> (rgb, info).  lit: None decides the light's visibility here; True / False takes it as given (the
        finite differences of the tolerance do not move a shadow)."""
        sh = self.shaders[node[2]]
        info = {}
        n0 = hit["normal"]
        M.decide(dot(d, n0), mpf(1), "faceforward")
        N = n0 if dot(d, n0) < 0 else neg(n0)            # rt/imported_types.d:69-73
        p = hit["p"]
        if sh[0] == "lambert":
            diffuse = self.tex_color(sh[1], hit["u"], hit["v"], M, info)
        else:
            diffuse = sh[1]
        if lit is None:
            start = add(p, scl(N, -self.e6 if "shadow_offset_minus_n" in self.mis else self.e6))
            lit, blocker = self.visible(start, self.light_pos, M)
            info["blocker"] = blocker
        info["lit"] = lit
        contrib = list(self.ambient)
        spec = [mpf(0)] * 3
        if lit:
            ldir = unit(sub(self.light_pos, p))
            cos_theta = dot(ldir, N)
            M.decide(cos_theta, mpf(1), "cosTheta")
            base = tuple(c * self.light_power / dot(sub(p, self.light_pos), sub(p, self.light_pos)) for c in self.light_color)
            info["cos_theta"] = cos_theta
            if sh[0] == "lambert":
                if cos_theta > 0:
                    contrib = [a + b * cos_theta for a, b in zip(contrib, base)]
            else:
                if cos_theta > 0:
                    contrib = [a + b * cos_theta for a, b in zip(contrib, base)]
                ray = neg(ldir)                          # reflect(-lightDir, N), rt/imported_types.d:62-67
                if "reflect_sign" in self.mis:
                    R = unit(add(ray, scl(N, 2 * dot(ray, N))))
                else:
                    R = unit(sub(ray, scl(N, 2 * dot(ray, N))))
                cos_gamma = dot(R, neg(d))
                M.decide(cos_gamma, mpf(1), "cosGamma")
                info["cos_gamma"] = cos_gamma
                if cos_gamma > 0:
                    strength = mpf(1) if "no_strength" in self.mis else sh[3]
                    spec = [b * cos_gamma ** sh[2] * strength for b in base]
                    if "specular_times_material" in self.mis:
                        spec = [s * c for s, c in zip(spec, diffuse)]
        info["specular"] = spec
        return tuple(dc * c + s for dc, c, s in zip(diffuse, contrib, spec)), info

    def sample(self, x, y, M):
        """one ray through (x, y): everything the JSON records, as mpf"""
        d = self.screen_ray(x, y)
        node, hit = self.trace(self.cam_pos, d, M)
        out = {"dir": d, "node": None, "leaf": None, "rgb": (mpf(0), mpf(0), mpf(0)), "lit": None}
        out["box"] = self.box_crossing(d)
        if node is None:
            return out
        rgb, info = self.shade(node, d, hit, M)
        out.update(node=node[0], leaf=hit["g"], t=hit["dist"], p=hit["p"], normal=hit["normal"], u=hit["u"], v=hit["v"],
                   rgb=rgb, lit=info["lit"], info=info, hit=hit, node_tuple=node)
        return out

    def box_crossing(self, d):
        """category 5, stated without the CSG walk: does the camera ray cross the cube's box (slab test), and does
        the whole crossing [t_in, t_out] lie inside the ball of R 70?  A segment lies in a ball iff both ends do.
        -> None (misses the box) or (t_in, t_out, clearance of the farther end from the ball's surface)."""
        c, half = self.geoms["cube"][1], self.geoms["cube"][2] / 2
        o = self.cam_pos
        t_in, t_out = mpf(0), BIG
        for k in range(3):
            if d[k] == 0:
                if abs(o[k] - c[k]) > half:
                    return None
                continue
            a, b = ((c[k] - half) - o[k]) / d[k], ((c[k] + half) - o[k]) / d[k]
            t_in, t_out = max(t_in, min(a, b)), min(t_out, max(a, b))
        if t_in > t_out:
            return None
        sc, R = self.geoms["sphere"][1], self.geoms["sphere"][2]
        clear = min(R - norm(sub(add(o, scl(d, t)), sc)) for t in (t_in, t_out))
        return (t_in, t_out, clear)


def categorize(s):
    """the category of the table (and 'through': also category 5) of one sample, from this script's own decisions"""
    through = s["box"] is not None and s["box"][2] > 0 and s["node"] != "csgNode"
    if s["node"] is None:
        cat = "sky"
    elif s["node"] == "floor":
        cat = "floor_lit" if s["lit"] else ("floor_shadow_csg" if s["info"]["blocker"] == "csgNode" else "floor_shadow_other")
    elif s["node"] == "globe":
        cat = "globe"
    elif s["node"] in ("S1", "S2", "S3"):
        # blue material: red comes only from the highlight.  "On the highlight": the specular term is at least 0.5,
        # which is more than the diffuse blue of any ball pixel but the brightest
        sp = s["info"]["specular"][0]
        cat = "ball_highlight" if s["info"].get("cos_gamma", -1) > 0 and sp >= mpf("0.5") else "ball_" + s["node"]
    else:
        n = s["normal"]
        if s["leaf"] == "cube":
            cat = "cube_" + {(0, 0, -1): "-z", (0, 1, 0): "+y", (1, 0, 0): "+x"}.get(tuple(int(c) for c in n), "other")
        else:
            cat = "cavity_lit" if s["lit"] else "cavity_shadow"
    return cat, through


def survey(step):
    """python make_lecture5_anchors.py --survey STEP: category of every STEP-th pixel, to choose PIXELS from"""
    sc = Scene()
    for y in range(0, H, step):
        for x in range(0, W, step):
            M = Margins()
            s = sc.sample(x, y, M)
            cat, through = categorize(s)
            print(x, y, cat, int(through), "ok" if M.fail is None else "FRAGILE " + M.fail, float(s["rgb"][0]), flush=True)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--survey":
    survey(int(sys.argv[2]))
    sys.exit(0)

# ---- the anchored pixels: (x, y, category, seen through the cube's silhouette), chosen from --survey ----------------------
PIXELS = [
    (100, 4, "sky", False), (560, 8, "sky", False),
    (352, 252, "floor_lit", False), (472, 352, "floor_lit", False), (472, 412, "floor_lit", False),
    (256, 276, "floor_shadow_csg", False), (200, 376, "floor_shadow_csg", False),
    (144, 272, "floor_shadow_csg", True), (120, 268, "floor_shadow_csg", True),
    (392, 208, "floor_shadow_other", False), (476, 308, "floor_shadow_other", False), (516, 372, "floor_shadow_other", False),
    (144, 116, "floor_lit", True), (52, 188, "floor_lit", True), (32, 292, "floor_lit", True), (40, 208, "floor_lit", True),
    (72, 256, "floor_lit", True), (112, 328, "floor_lit", True), (144, 304, "floor_lit", True),
    (428, 120, "globe", False), (456, 132, "globe", False), (484, 164, "globe", False),
    (436, 240, "ball_S1", False), (456, 240, "ball_S1", False), (472, 276, "ball_S2", False), (480, 300, "ball_S2", False),
    (536, 336, "ball_S3", False), (500, 348, "ball_S3", False),
    (453, 233, "ball_highlight", False), (476, 270, "ball_highlight", False), (508, 324, "ball_highlight", False),
    (180, 176, "cube_-z", False), (200, 224, "cube_-z", False), (28, 328, "cube_-z", False),
    (68, 116, "cube_+y", False), (136, 164, "cube_+y", False),
    (208, 152, "cube_+x", False), (220, 316, "cube_+x", False),
    (128, 232, "cavity_lit", False), (160, 252, "cavity_lit", False), (80, 340, "cavity_lit", False),
    (112, 116, "cavity_shadow", False), (96, 184, "cavity_shadow", False), (100, 264, "cavity_shadow", False),
]
TAP_PIXELS = [(352, 252, "interior"), (213, 140, "silhouette"), (475, 236, "rim")]
# misreading -> (what it is, the pixels it applies to)
LIT = lambda a: a["lit"] is True
# the specular term is there and fp32 holds it as a normal number: the channel that carries only the highlight (red of
# the blue balls, blue of the yellow cube) then pins it to the channel's RELATIVE tolerance, on or off the highlight
HIGHLIGHT = lambda a: a.get("specular", 0) >= 1e-30
# at the very peak cosGamma -> 1 and cosGamma ^^ n does not depend on n: the exponent is pinned on the flank
FLANK = lambda a: HIGHLIGHT(a) and a["cos_gamma"] <= 0.995
# from p - N * 1e-6 a plane or a sphere hits itself at once.  The CsgDiff does not: the ray starts INSIDE the solid, the
# walk of rt/geometry.d:306-329 starts from the parities and reports only a hit at which boolOp becomes true, and
# leaving the solid is not one; a lit pixel of csgNode stays lit, so it cannot tell the two signs apart
LIT_NOT_CSG = lambda a: a["lit"] is True and a["node"] != "csgNode"
MISREADINGS = {
    "no_flip": ("cavity normal not flipped", lambda a: a["category"].startswith("cavity")),
    "reflect_sign": ("reflect with the opposite sign", HIGHLIGHT),
    "exp79": ("Phong exponent one less (79 for the balls, 59 for the cube)", FLANK),
    "exp81": ("Phong exponent one more (81 for the balls, 61 for the cube)", FLANK),
    "no_strength": ("strength dropped from the specular term", HIGHLIGHT),
    "specular_times_material": ("specular multiplied by the material colour", HIGHLIGHT),
    "shadow_offset_minus_n": ("shadow ray leaving p - N * 1e-6", LIT_NOT_CSG),
    "sphere_v_no_one_minus": ("sphere v without the `1 -`", lambda a: a["leaf"] in ("globe_ball", "S", "sphere")),
    "sphere_u_atan2_xz": ("sphere u from atan2(x, z)", lambda a: a["leaf"] in ("globe_ball", "S", "sphere")),
    "cube_uv_unpermuted": ("cube side faces with u, v = (x, z) as on the Y faces", lambda a: a["category"] in ("cube_-z", "cube_+x")),
    "root_swap": ("x1 / x2 swapped in Sphere.intersect", lambda a: a["leaf"] in ("globe_ball", "S", "sphere")),
    "rows_top_down": ("texture rows read top-down", lambda a: a["node"] in ("floor", "globe")),
    "no_srgb": ("sRGB decode skipped", lambda a: a["node"] in ("floor", "globe")),
    "scaling_divides": ("floor scaling applied as a divisor", lambda a: a["node"] == "floor"),
}
TAP_MISREADINGS = {
    "aa_divisor_4": "the five taps divided by 4",
    "aa_offsets_quarter_half": "tap offsets 0.25 / 0.5 in place of 0.3 / 0.6",
    "aa_offsets_half_threequarter": "tap offsets 0.5 / 0.75 in place of 0.3 / 0.6",
}
REQUIRED = ("sky", "floor_lit", "floor_shadow_csg", "floor_shadow_other", "globe", "ball_S1", "ball_S2", "ball_S3",
            "ball_highlight", "cube_-z", "cube_+y", "cube_+x", "cavity_lit", "cavity_shadow")
GEOM_KEYS = ("dir", "t", "p", "normal", "u", "v")
CAP = 1e12                                               # ratios are stored capped: a changed branch counts as this


def ulp64(m):
    return mpf(2) ** (int(floor(mp.log(m, 2))) - 52)


def as_list(v):
    return list(v) if isinstance(v, (tuple, list)) else [v]


def fl(v):
    if v is None or isinstance(v, (bool, str, int)):
        return v
    return [float(x) for x in v] if isinstance(v, (tuple, list)) else float(v)


def anchor(x, y):
    """one sample with everything the JSON holds: values (50 digits), tolerances, and the robustness verdict"""
    sc, M = Scene(), Margins()
    s = sc.sample(x, y, M)
    with workprec(53):
        s53 = Scene().sample(x, y, Margins())
    assert (s53["node"], s53["leaf"], s53["lit"]) == (s["node"], s["leaf"], s["lit"])
    cat, through = categorize(s)
    a = {"x": fl(x), "y": fl(y), "category": cat, "through_cube_silhouette": through, "node": s["node"], "leaf": s["leaf"],
         "lit": s["lit"], "specular_share": None}
    problems = [M.fail] if M.fail else []
    tol = {}
    sphere_leaf = s["leaf"] in ("globe_ball", "S", "sphere")
    for k in GEOM_KEYS:
        if k != "dir" and s["node"] is None:
            a[k] = None
            continue
        if k in ("dir", "normal") or (k in ("u", "v") and sphere_leaf):
            mag, cap = (mpf(8) if k in ("u", "v") else mpf(1)), mpf("1e-12")      # PI + angle < 2 PI < 8
        else:
            leafc = sc.geoms[s["leaf"]][1] if s["leaf"] != "floor" else (mpf(0),) * 3
            mag = max([abs(c) for c in s["p"] + sc.cam_pos + leafc + s["node_tuple"][3]] + [s["t"]])
            cap = mpf("1e-9")
        d = max(abs(p - q) for p, q in zip(as_list(s[k]), as_list(s53[k])))
        tol[k] = max(16 * d, 8 * ulp64(mag))
        if tol[k] > cap:
            problems.append("geometry cap: tolerance %s of %s over %s" % (mp.nstr(tol[k], 3), k, mp.nstr(cap, 3)))
        a[k], a[k + "_tol"] = fl(s[k]), float(tol[k])
    rgb = s["rgb"]
    if s["node"] is None:
        rgb_tol = (mpf(0),) * 3
    else:
        kk = K_PHONG if sc.shaders[s["node_tuple"][2]][0] == "phong" else K_LAMBERT_BITMAP
        push = [mpf(0)] * 3
        quiet = Margins()
        for k in ("dir", "p", "normal", "u", "v"):
            for i in range(len(as_list(s[k]))):
                hit, d = dict(s["hit"]), s["dir"]
                if k == "dir":
                    d = tuple(c + (tol[k] if j == i else 0) for j, c in enumerate(d))
                elif k in ("u", "v"):
                    hit[k] = hit[k] + tol[k]
                else:
                    hit[k] = tuple(c + (tol[k] if j == i else 0) for j, c in enumerate(hit[k]))
                moved, _ = sc.shade(s["node_tuple"], d, hit, quiet, lit=s["lit"])
                push = [pp + abs(m - c) for pp, m, c in zip(push, moved, rgb)]
        rgb_tol = tuple(2 * kk * (EPS24 * c + mpf(2) ** -149) + pp for c, pp in zip(rgb, push))
        for c, t in zip(rgb, rgb_tol):
            if t > mpf("5e-6") * max(1, c):
                problems.append("colour tolerance %s over the cap" % mp.nstr(t, 3))
        info, hit = s["info"], s["hit"]
        a["specular"] = float(info["specular"][0])
        if info["specular"][0] > 0:
            a["specular_share"] = float(info["specular"][0] / max(rgb))
        if "cos_gamma" in info:
            a["cos_gamma"] = float(info["cos_gamma"])
        if "texel" in info:
            a["texel"], a["bilinear_pq"] = info["texel"], fl(info["bilinear_pq"])
        if not s["lit"]:
            a["blocker"] = info["blocker"]
        if "flipped" in hit:
            a["normal_flipped"], a["csg_hits"] = hit["flipped"], hit["csg"]
        if s["node"] in ("S1", "S2", "S3"):
            a["object_space"] = {"orig": fl(hit["orig_object"]), "t": fl(hit["dist_object"]), "p": fl(hit["p_object"])}
    a["rgb"], a["rgb_tol"] = fl(rgb), fl(rgb_tol)
    return a, s, problems, M


def check_category(a, s):
    """what the table of categories makes the generator assert, beyond the name of the category"""
    cat, sc = a["category"], Scene()
    if cat == "sky":
        assert s["node"] is None and a["rgb"] == [0.0, 0.0, 0.0]
    if a["through_cube_silhouette"]:
        # the ray meets the box, both ends of the crossing are inside the ball, and the CSG walk of THIS script
        # (independent of box_crossing) returned no hit on the node: whatever is closest is not csgNode
        t_in, t_out, clear = s["box"]
        assert t_in < t_out and clear > mpf("1e-3") and s["node"] != "csgNode"
        d = s["dir"]
        assert sc.node_hit(sc.nodes[2], sc.cam_pos, d, BIG, Margins(), False) is None
        a["box_t"], a["ball_clearance"] = [float(t_in), float(t_out)], float(clear)
    if cat.startswith("floor"):
        assert s["node"] == "floor" and s["leaf"] == "floor" and a["normal"] == [0.0, 1.0, 0.0]
        scaling = sc.textures["bmp"][1]
        for coord, size, got in ((s["u"], 256, a["texel"][0]), (s["v"], 256, a["texel"][1])):
            t = coord * scaling
            assert int(floor((t - floor(t)) * size)) == got
        assert a["lit"] == (cat == "floor_lit")
        if cat == "floor_shadow_csg":
            assert a["blocker"] == "csgNode"
        if cat == "floor_shadow_other":
            assert a["blocker"] in ("globe", "S1", "S2", "S3")
        if not a["lit"]:                                 # texture * ambient only
            diffuse = sc.tex_color("bmp", s["u"], s["v"], Margins(), {})
            assert all(abs(c - dd * am) < mpf("1e-40") for c, dd, am in zip(s["rgb"], diffuse, sc.ambient))
    if cat == "globe":
        assert s["node"] == "globe" and s["leaf"] == "globe_ball" and 0 < s["u"] < 1 and 0 < s["v"] < 1 and "texel" in a
    if cat.startswith("ball"):
        node = s["node_tuple"]
        assert node[0] in ("S1", "S2", "S3") and s["leaf"] == "S"
        h = s["hit"]
        assert h["orig_object"] == sub(sc.cam_pos, node[3]) and h["p"] == add(h["p_object"], node[3])
        assert abs(norm(h["p_object"]) - 15) < mpf("1e-40") and abs(h["dist"] - norm(sub(h["p"], sc.cam_pos))) < mpf("1e-40")
        if cat == "ball_highlight":
            assert a["cos_gamma"] > 0 and 2 * a["specular"] >= a["rgb"][0] and a["specular"] >= 0.5
        else:
            assert cat == "ball_" + node[0] and a["specular"] < 1e-3                       # away from the highlight
    if cat.startswith("cube"):
        c = sc.geoms["cube"][1]
        rel = sub(s["p"], c)
        want = {"cube_-z": ((0, 0, -1), rel[0], rel[1]), "cube_+y": ((0, 1, 0), rel[0], rel[2]), "cube_+x": ((1, 0, 0), rel[1], rel[2])}[cat]
        assert s["leaf"] == "cube" and tuple(int(v) for v in s["normal"]) == want[0] and s["u"] == want[1] and s["v"] == want[2]
        assert a["normal_flipped"] is False
    if cat.startswith("cavity"):
        c = sc.geoms["sphere"][1]
        assert s["leaf"] == "sphere" and a["normal_flipped"] is True
        assert dot(s["normal"], sub(s["p"], c)) < 0 and dot(s["normal"], s["dir"]) < 0     # towards the centre and the eye
        assert abs(s["t"] - (norm(sub(s["p"], sc.cam_pos)) - sc.e6)) < mpf("1e-40")        # the second hit of the ball
        assert a["lit"] == (cat == "cavity_lit")


def ratio(a, mis):
    """largest |misread - anchor| / tolerance over the recorded quantities of one anchored sample"""
    try:
        with workprec(mp.prec):
            s = Scene(mis).sample(a["x"], a["y"], Margins())
    except (AssertionError, ZeroDivisionError, ValueError):
        return CAP
    if (s["node"], s["leaf"], s["lit"]) != (a["node"], a["leaf"], a["lit"]):
        return CAP
    worst = mpf(0)
    for k in GEOM_KEYS + ("rgb",):
        if a[k] is None:
            continue
        tols = as_list(a[k + "_tol"]) if k == "rgb" else [a[k + "_tol"]] * 3
        for got, want, t in zip(as_list(s[k]), a[k] if isinstance(a[k], list) else [a[k]], tols):
            if t > 0:
                worst = max(worst, abs(got - mpf(want)) / mpf(t))
            elif got != want:
                return CAP
    return float(min(worst, CAP))


def tap_anchor(x, y, taps=TAPS, divisor=5):
    samples = []
    for dx, dy in taps:
        a, s, problems, M = anchor(x + dbl(dx), y + dbl(dy))
        # a tap must be robust and hold the colour cap; the caps on t, p, normal, u, v are for the probed pixels (a tap's
        # geometry is not compared, and its geometry tolerance is already inside its colour tolerance)
        samples.append((a, s, [p for p in problems if not p.startswith("geometry cap")]))
    mean = [sum(mpf(a["rgb"][k]) for a, _, _ in samples) / divisor for k in range(3)]
    tol = [sum(mpf(a["rgb_tol"][k]) for a, _, _ in samples) / 5 + K_AA * EPS24 * mean[k] for k in range(3)]
    return samples, mean, tol


def build():
    sc = Scene()
    out = {
        "source": "tests/golden/make_lecture5_anchors.py: the reference's algorithm (rt/camera.d:77-147, rt/node.d:24-47, "
                  "rt/geometry.d:30-59,92-125,172-235,271-332,382-397, rt/shader.d:67-105,197-250, rt/scene.d:62-78, "
                  "rt/texture.d:117-128, rt/bitmap.d:48-63,116-126, rt/renderer.d:233-251) restated in 50-digit arithmetic; "
                  "NOT reference output, NOT oracle / host-mirror / kernel output",
        "scene": "lecture5.sdl", "width": W, "height": H, "dof": 0,
        "nodes": [n[0] for n in sc.nodes], "geometries": list(sc.geoms),
        "node_geometry": {n[0]: n[1] for n in sc.nodes},
        "camera": {k: fl(getattr(sc, k)) for k in ("up_left", "up_right", "down_left", "right_dir", "up_dir", "front_dir")},
        "fp32_roundings": {"lambert_bitmap": K_LAMBERT_BITMAP, "phong": K_PHONG, "aa_mean": K_AA},
        "background": [0.0, 0.0, 0.0],
    }
    out["camera"]["tolerance"] = 1e-13
    worst = Margins()
    pixels = []
    for (x, y, cat, through) in PIXELS:
        a, s, problems, M = anchor(x, y)
        assert not problems, (x, y, problems)
        assert (a["category"], a["through_cube_silhouette"]) == (cat, through), (x, y, a["category"], a["through_cube_silhouette"])
        check_category(a, s)
        for k, v in M.worst.items():
            worst.worst[k] = min(worst.worst[k], v)
        pixels.append(a)
    cats = [a["category"] for a in pixels]
    assert all(c in cats for c in REQUIRED), [c for c in REQUIRED if c not in cats]
    assert sum(a["through_cube_silhouette"] for a in pixels) >= 4
    out["pixels"] = pixels
    taps_out = []
    for (x, y, kind) in TAP_PIXELS:
        samples, mean, tol = tap_anchor(x, y)
        for a, s, problems in samples:
            assert not problems, (x, y, a["x"], a["y"], problems)
        kinds = sorted({a["category"] for a, _, _ in samples})
        assert (kind == "interior") == (len(kinds) == 1), (x, y, kinds)
        assert all(t <= mpf("5e-6") * max(1, m) for t, m in zip(tol, mean))
        taps_out.append({"x": x, "y": y, "kind": kind, "categories": kinds,
                         "taps": [{k: a[k] for k in ("x", "y", "category", "node", "leaf", "rgb", "rgb_tol")} for a, _, _ in samples],
                         "mean": fl(mean), "mean_tol": fl(tol)})
    out["five_tap"] = taps_out
    out["smallest_margins"] = {k: float(v) for k, v in worst.worst.items()}
    # ---- the misreadings ----
    ratios, loose = {}, {}
    for name, (what, applies) in MISREADINGS.items():
        rs = [ratio(a, (name,)) for a in pixels if applies(a)]
        if name == "no_strength":
            assert all(sh[3] == 1 for sh in sc.shaders.values() if sh[0] == "phong")
        entry = {"what": what, "pixels": len(rs), "min_ratio": min(rs) if rs else 0.0}
        (ratios if rs and min(rs) >= 100 else loose)[name] = entry
    for name, what in TAP_MISREADINGS.items():
        rs = []
        for t in taps_out:
            if name == "aa_divisor_4":
                _, mean, _ = tap_anchor(t["x"], t["y"], divisor=4)
            else:
                m = {"0.3": "0.25", "0.6": "0.5"} if name == "aa_offsets_quarter_half" else {"0.3": "0.5", "0.6": "0.75"}
                _, mean, _ = tap_anchor(t["x"], t["y"], taps=tuple((m.get(dx, dx), m.get(dy, dy)) for dx, dy in TAPS))
            rs.append(float(min(max(abs(m - mpf(w)) / mpf(tt) for m, w, tt in zip(mean, t["mean"], t["mean_tol"]) if tt > 0), CAP)))
        entry = {"what": what, "pixels": len(rs), "min_ratio": min(rs)}
        (ratios if min(rs) >= 100 else loose)[name] = entry
    out["misreadings"] = ratios
    reasons = {"no_strength": "lecture5.sdl gives no strength, so both Phong shaders hold the default 1.0f (rt/shader.d:177-195): "
                              "multiplying by it or not is the same value; only a scene with strength != 1 can tell"}
    assert set(loose) <= set(reasons), loose
    out["not_constrained"] = {k: dict(v, reason=reasons[k]) for k, v in loose.items()}
    return out


def main():
    out = build()
    with open(os.path.join(HERE, "lecture5_anchors.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote lecture5_anchors.json:", len(out["pixels"]), "pixels,", len(out["five_tap"]), "five-tap anchors")
    for a in out["pixels"]:
        print(a["x"], a["y"], a["category"], int(a["through_cube_silhouette"]), a["rgb"], max(a["rgb_tol"]))
    for k, v in out["misreadings"].items():
        print("%-30s min ratio %.3g over %d" % (k, v["min_ratio"], v["pixels"]))
    print("not constrained:", list(out["not_constrained"]), " margins:", out["smallest_margins"])


if __name__ == "__main__":
    main()

/*
 * c2rt_trace_shared.inc — the half of the trace that does not depend on the arithmetic mode: table pointer types,
 * vectors, the window accumulator, hit records, Ctx, CSG tags and node walk, u,v, textures, RNG, pixel output.
 *
 * Included ONCE by c2rt_trace_common.inc, inside c2rt::{anonymous} and in front of namespaces lean:: and exact::,
 * which both read these definitions unqualified; so do the kernels and the query files.  The rule: a definition
 * lives here if it does not read kLean and does not call or instantiate anything of c2rt_trace.inc (which is what
 * the two namespaces hold).  In the order the trace uses them.
 */
/* The scene tables (nodes, geometries, lights, textures' records) are read through CONSTANT-address-space
 * pointers: nothing writes them while a frame renders, and a load through such a pointer whose address is
 * wave-uniform is a scalar load (s_load: the record lives in SGPRs) whatever global stores and atomics the kernel
 * holds.  Through a generic pointer the compiler has to prove that no store of the kernel can have clobbered
 * the location; where it cannot (every record read after the first store or atomic, and everything whose address
 * derives from such a read: the child indices of a CsgOp, its children's records, ...) the record comes through
 * vector loads into VGPRs, with a full memory latency per link of the chain.  A per-lane address (the leaf
 * under a CsgOp in hit_surface) is a vector load either way. */
#define C2RT_K __attribute__((address_space(4)))
typedef const DevGeom C2RT_K *GeomP;
typedef const DevNode C2RT_K *NodeP;
typedef const DevLight C2RT_K *LightP;
typedef const DevTex C2RT_K *TexP;
typedef const DevMat C2RT_K *MatP;
typedef const double C2RT_K *KDbl;
typedef const float C2RT_K *KFlt;

/* Diagnostics build only (-DC2RT_TILE_STATS=1, scripts/tile_stats.py): where a wave's time goes and how full the wave
 * is when it gets there — per region {shader-clock ticks between BEGIN and END, lanes active at BEGIN, 64 per entry},
 * accumulated over the frame behind the per-tile stamps (Ctx::lane_stats + 4 + 3 * id).  END sits where the lanes
 * that entered are active again.  The product build compiles both macros to nothing. */
#if C2RT_TILE_STATS
enum { kRegTrace = 0, kRegCsg = 1, kRegReplay = 2, kRegSurface = 3, kRegShade = 4, kRegShadow = 5, kRegTexture = 6, kRegLight = 7, kRegSphereUV = 8, kRegions = 9 };
#define C2RT_REGION_BEGIN(cx, id)                                                                          \
    const unsigned long long rs_##id = (cx).lane_stats ? __builtin_amdgcn_s_memtime() : 0ull;              \
    const unsigned long long ra_##id = __ballot(true);
#define C2RT_REGION_END(cx, id)                                                                            \
    if ((cx).lane_stats) {                                                                                 \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                      \
        if ((cx).lane == (int)__builtin_ctzll(__ballot(true))) {                                           \
            atomicAdd((cx).lane_stats + 4 + 3 * (id) + 0, now_ - rs_##id);                                 \
            atomicAdd((cx).lane_stats + 4 + 3 * (id) + 1, (unsigned long long)__builtin_popcountll(ra_##id)); \
            atomicAdd((cx).lane_stats + 4 + 3 * (id) + 2, 64ull);                                          \
        }                                                                                                  \
    }
#else
#define C2RT_REGION_BEGIN(cx, id)
#define C2RT_REGION_END(cx, id)
#endif

/* ------------------------------------------------------------------ */
/* small vector types (gfm vec3d / rt Color semantics)                  */
/* ------------------------------------------------------------------ */

struct D3 { double x, y, z; };
DEV D3 mk(double x, double y, double z) { D3 r; r.x = x; r.y = y; r.z = z; return r; }
DEV D3 ld3(const double *p) { return mk(p[0], p[1], p[2]); }
DEV D3 ld3(KDbl p) { return mk(p[0], p[1], p[2]); }
DEV D3 operator+(D3 a, D3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
DEV D3 operator-(D3 a, D3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
DEV D3 operator*(D3 a, double s) { return mk(a.x * s, a.y * s, a.z * s); }
DEV D3 operator-(D3 a) { return mk(-a.x, -a.y, -a.z); }
/* gfm dot/squaredMagnitude start from `sum = 0`; 0 + x differs from x only in
 * the sign of an exact zero, which no consumer on this path observes. */
DEV double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
DEV double sqmag(D3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
DEV double mag(D3 a) { return sqrt(sqmag(a)); }

/* The out-of-window accumulator (Ctx::bad): every lean divide / sqrt folds its operand's exponent test into
 * it with three 32-bit instructions (two for a sum of squares) and no compare, branch or scalar instruction — in_window's
 * t = (hi & 0x7FFFFFFF) - (LO << 20) is below SPAN << 20 exactly for finite operands in [2^LO, 2^HI), so the
 * running unsigned MAXIMUM of t over everything the lane divided or took the root of is below it iff all of
 * them were.  One window serves every site, [2^-240, 2^240) (1e-72 .. 1e+72): it is the square of den_ok's,
 * so that a length taken from a checked sum of squares is a valid denominator, and far inside num_ok's. */
struct Oob {
    uint32_t t;
};
constexpr int kWinLo = -240, kWinHi = 240;
DEV void oob_init(Oob &b) { b.t = 0; }
/* t in units of the high word itself (exponent at bit 20): sign masked off, low bound subtracted, running
 * maximum — three instructions.  (Written as `(hi << 1) - (LO << 21)` the compiler extracts the shifted word
 * with a 64-bit shift by 31 and a mask, v_alignbit_b32 + v_and_b32: four; that form was a build switch up to
 * commit f0eed4f.)  The first instruction is spelled out so that the high word stays a 32-bit value of its own. */
constexpr int kOobShift = 20;
DEV void oob_note(Oob &b, double x)
{
    uint32_t m;
    asm("v_and_b32_e32 %0, 0x7fffffff, %1" : "=v"(m) : "v"(__double2hiint(x)));
    const uint32_t t = m - ((uint32_t)(kWinLo + 1023) << 20);
    b.t = b.t > t ? b.t : t;
}
/* the same for an operand that cannot be negative (a sum of squares): no mask — two instructions; a set sign
 * bit reads as out of window, which only costs a redo */
DEV void oob_note_nonneg(Oob &b, double x)
{
    uint32_t t;
    asm("v_subrev_u32_e32 %0, %2, %1" : "=v"(t) : "v"(__double2hiint(x)), "n"((uint32_t)(kWinLo + 1023) << 20));
    b.t = b.t > t ? b.t : t;
}
DEV bool oob_any(const Oob &b) { return b.t >= ((uint32_t)(kWinHi - kWinLo) << kOobShift); }
/* an fp32 operand (window 2^+-60, fp64_lean.h: f32_ok) folded into the same accumulator: outside -> all ones */
DEV void oob_note_f32(Oob &b, float x)
{
    const uint32_t t = f32_ok(x) ? 0u : 0xFFFFFFFFu;
    b.t = b.t > t ? b.t : t;
}

/* mul(v, M): row vector x matrix — rt/imported_types.d:13-20 */
DEV D3 mulvm(D3 v, KDbl m)
{
    return mk(v.x * m[0] + v.y * m[3] + v.z * m[6],
              v.x * m[1] + v.y * m[4] + v.z * m[7],
              v.x * m[2] + v.y * m[5] + v.z * m[8]);
}

struct F3 { float r, g, b; };
DEV F3 mkf(float r, float g, float b) { F3 c; c.r = r; c.g = g; c.b = b; return c; }
DEV F3 ldf3(const float *p) { return mkf(p[0], p[1], p[2]); }
DEV F3 ldf3(KFlt p) { return mkf(p[0], p[1], p[2]); }
DEV F3 operator+(F3 a, F3 b) { return mkf(a.r + b.r, a.g + b.g, a.b + b.b); }
DEV F3 operator*(F3 a, F3 b) { return mkf(a.r * b.r, a.g * b.g, a.b * b.b); }
DEV F3 operator*(F3 a, float f) { return mkf(a.r * f, a.g * f, a.b * f); }
DEV F3 operator/(F3 a, float f) { return mkf(a.r / f, a.g / f, a.b / f); }

/* x86 cvttsd2si / cvttss2si results for out-of-range inputs, which is what
 * the reference binary computes for cast(int) / cast(size_t). */
DEV int d2i_x86(double d)
{
    return (d > -2147483649.0 && d < 2147483648.0) ? (int)d : (int)0x80000000;
}

/* ------------------------------------------------------------------ */
/* hit record                                                           */
/* ------------------------------------------------------------------ */

/* What the trace keeps of an IntersectionData (rt/intersectable.d:6-33) while it looks for the closest
 * hit: the point (in the object space of the node under test), the distance, the LEAF geometry and three
 * bits.  Normal, u, v (and dNdx / dNdy, dead on this path) are functions of exactly these — Plane: constants
 * and p; Cube: the face and p - center; Sphere: p - center — so they are evaluated ONCE, for the closest
 * hit of the sample, after the node loop (hit_surface), with the operations the reference applies to every
 * candidate: the same bits, a record of 10 registers instead of 24 through the whole trace, and no
 * normalisation / division for candidates that lose. */
struct Hit {
    D3 p;
    double dist;
    int g;
    int code;         /* kCodeAxis: Cube face axis, kCodeSide: its +side, kCodeFlip: CsgDiff negated the normal an odd number of times */
};
enum { kCodeAxis = 3, kCodeSide = 4, kCodeFlip = 8 };

/* the closest hit as the shaders read it (world space) */
struct Surf {
    D3 p, n;
    double u, v; /* a sphere's under kUVBitmap: good for bitmap_color's float conversion only, not the reference's doubles (UVWant) */
};

/* what a caller needs back from an intersect call */
enum Need {
    kBool = 0,  /* hit / no hit (and the distance) */
    kPoint = 1, /* + p and the leaf geometry */
    kFull = 2,  /* + the face / flip code the normal is rebuilt from (hit_surface) */
    kRt = 3     /* kPoint, and kFull for the lanes whose run-time `full` flag is set */
};
#define C2RT_WANT_FULL(NEED, full) ((NEED) == kFull || ((NEED) == kRt && (full)))

/* what the trace needs below the shading level: table bases (SGPRs), the
 * wave's CSG slabs and the lane.  Deliberately NOT a pointer to the kernel
 * arguments (which would have to be materialised in scratch if it escaped). */
/* The kernel-argument segment (the by-value RenderParams block), as handed down from the __global__
 * entry point: helpers must not fetch it themselves (__builtin_amdgcn_kernarg_segment_ptr() is only
 * meaningful in the kernel function; an out-of-line callee would read garbage). */
typedef const RenderParams __attribute__((address_space(4))) *KArgs;

/* The same for a batch kernel (frames, hit planes, adaptive refinement), whose parameter blocks are a table in HBM with
 * blockIdx.y = frame: block blockIdx.y of the table through a constant-address-space pointer — scalar loads, no VGPR,
 * exactly as a single-frame kernel re-reads its kernel-argument segment.  The pointer goes through an empty asm so
 * that the optimiser cannot fold the address-space casts back to the global pointer it was made from (loads through
 * that one would be vector loads: the kernel stores to global memory, so nothing proves them invariant). */
DEV KArgs batch_block(const RenderParams *table)
{
    KArgs K = (KArgs)table + blockIdx.y;
    asm volatile("" : "+s"(K));
    return K;
}

struct Ctx {
    KArgs kargs;
    GeomP geoms;
    NodeP nodes;
    uint32_t n_nodes;
    char *lds;        /* this wave's CSG hit stack: dist[csg_cap][64] (8 B) then tag[csg_cap][64] (2 B) */
    int lane;
    int csg_cap;      /* entries of that stack (wave-uniform, RenderParams::csg_cap) */
    /* A lane's nested hit lists did not fit csg_cap entries: its results are void and the whole tile is
     * rendered again by the full-capacity launch (RenderParams::retry_list).  Written through const
     * references on purpose: everything here is inlined into the kernel and it lives in a register. */
    mutable bool overflow;
    /* lean:: — whether some divide / sqrt of this lane met an operand outside the window (Oob): the lane's
     * results are then void and the tile is rendered again through exact:: (render_tile) */
    mutable Oob bad;
    /* Where a child's hit list reaches C2RT_MAX_CSG_HITS — the reference's findAllIntersections
     * (`while (true)`, rt/geometry.d:271-290) would have gone on, this build stops: build-defined
     * behaviour — the lane bumps this counter (c2rt_get_csg_truncations), so that nobody has to take
     * the cap's harmlessness on trust.  Null (at compile time) in the production instances: only the
     * instances launched when rays are being counted carry it (render_tile's CNT) — measured in the
     * headline kernel, which sits exactly at its 128-VGPR budget, a flag carried to the end of the tile
     * cost 3 % and an atomic on the spot 8 %. */
    unsigned long long *trunc_counter;
    /* a kCsgCertain CsgOp may be decided by csg_certain.h (csg_intersect_leaf).  A compile-time constant wherever it is
     * set: true in the uncounted frame instances, false in the counted ones — which therefore compare the two routes
     * bit for bit in every counted frame — and in the query kernels. */
#if C2RT_CSG_CERTAIN
    bool csg_certain;
#endif
#if C2RT_TILE_STATS
    unsigned long long *lane_stats; /* diagnostics: {active, slots} pairs — [0..1] CSG evaluations entered, [2..3] child stepping calls */
#endif
    uint32_t block;   /* the tile this wave renders (blockIdx.x, or an entry of the retry list) */
    uint32_t mask_slot; /* its entry in RenderParams::tile_masks (multi-light instances: light_shadow_mask) */
    uint32_t primary_mask; /* bit n clear: no primary ray of this tile can reach node n (wave-uniform) */
    uint32_t shadow_mask0; /* same for the tile's shadow rays towards light 0 (further lights: shadow_cull_mask) */
    /* the ground plane (RenderParams::ground_node) is the ONLY node left in shadow_mask0: the tile's
     * shadow rays towards light 0 are decided by plane_points_away alone, without building a ray */
    bool shadow_ground_only;
    /* the ground plane is the ONLY node left in primary_mask: the tile's primary rays take the
     * straight-line ground trace (raytrace) instead of the node loop */
    bool primary_ground_only;
    double ground_y;
};

/* The context of a lane that traces outside a frame tile (the pixel probe and the query kernels: caller's rays, hit
 * planes, adaptive refinement): no culling — every mask all ones —, no ground shortcut, nothing counted. */
DEV void query_ctx(Ctx &cx, const RenderParams &P, KArgs K, char *lds, int lane)
{
    cx.geoms = (GeomP)P.geoms;
    cx.nodes = (NodeP)P.nodes;
    cx.n_nodes = P.n_nodes;
    cx.kargs = K;
    cx.lds = lds;
    cx.lane = lane;
    cx.csg_cap = (int)P.csg_cap;
    cx.overflow = false;
    oob_init(cx.bad);
    cx.trunc_counter = nullptr;
#if C2RT_CSG_CERTAIN
    cx.csg_certain = false;
#endif
#if C2RT_TILE_STATS
    cx.lane_stats = nullptr;
#endif
    cx.block = 0;
    cx.mask_slot = 0;
    cx.primary_mask = 0xFFFFFFFFu;
    cx.shadow_mask0 = 0xFFFFFFFFu;
    cx.shadow_ground_only = false;
    cx.primary_ground_only = false;
    cx.ground_y = 0;
}

/* util.array.sort's next gap, `gap == 2 ? 1 : cast(int)(gap * 5.0 / 11)` (util/array.d:108): a list holds at
 * most 2 * kMaxCsgHits = 16 entries, so gap <= 8, and for such integers the truncated double quotient equals
 * the integer quotient (5 gap / 11 is never within rounding of an integer unless 11 divides gap) — one
 * multiply-shift instead of an fp64 division per sorting pass. */
DEV int next_gap(int inc)
{
    static_assert(2 * kMaxCsgHits <= 22, "gap * 5 / 11 in integers");
    return inc == 2 ? 1 : (inc * 5) / 11;
}

/* hit-list tag: leaf geometry (12 bits: C2RT_MAX_CSG_GEOMS) | child side | index of the hit in its child's list.
 * In a CsgOp over two primitives (csg_intersect_leaf) the leaf IS the child, which the side bit names: the upper field
 * carries the hit's face code (kCodeAxis | kCodeSide) instead, for winners that need no replay. */
static_assert(kMaxCsgHits <= 8 && C2RT_MAX_CSG_GEOMS <= 4096, "16-bit hit tags");
DEV uint16_t csg_tag(int leaf, int side, int k) { return (uint16_t)(((uint32_t)leaf << 4) | ((uint32_t)side << 3) | (uint32_t)k); }

/* The first node >= n that a culling mask keeps: bit k of `mask` clear means
 * node k (< kMaxCullNodes = 32) cannot be reached; nodes beyond the mask are
 * always visited.  Wave-uniform: a shift and a find-first-set on the scalar unit. */
DEV uint32_t next_node(uint32_t mask, uint32_t n)
{
    static_assert(kMaxCullNodes == 32, "one 32-bit mask");
    if (n >= 32u) return n;
    const uint32_t m = mask >> n;
    return m ? n + (uint32_t)__builtin_ctz(m) : 32u;
}

/*
 * Plane.intersect's first rejection (rt/geometry.d:33-34: origin above the plane
 * and direction not pointing down, or the mirror image), decided from the
 * UN-normalised direction `raw` of a ray that would be traced as
 * make_ray(from, normalized(raw)) against an "axis plane" node (kNodeAxisPlane:
 * a Plane whose inverse matrix is the identity, or diagonal with entries of
 * magnitude in [1e-100, 1e100] and a positive y entry b).
 * With raw.y in (1e-150, 1e150) and |raw.x|, |raw.z| < 1e150:
 *   |raw|^2 is a positive normal number, 1/|raw| is positive, finite and normal,
 *   dir.y = raw.y / |raw| > 5e-301, dir is finite and |dir| is within rounding of 1;
 *   identity matrix: the node test sees dn.y = dir.y * (1/|dir|), a positive number;
 *   diagonal matrix: it sees dd = dir . inv, dd.y = (+-0) + dir.y * b + (+-0) >= 0 (possibly
 *   underflowed to zero), |dd| in [0.5e-100, 1.1e100], and d'.y = dd.y * (1/|dd|) >= 0, not NaN;
 *   either way `d.y > -1e-9` holds, and with o'.y > y the reference returns false.
 * (Mirror image for raw.y < 0 and o'.y < y.)  o'.y is evaluated literally.  Outside
 * those bounds — zero, huge, infinite or NaN components — the answer is "don't
 * know" and the literal evaluation runs.  What this saves: both normalisations
 * (2 sqrt, 2 divisions) and the matrix products of every ray that hits nothing.
 * Used by the kernel instances for scenes made of such planes only (PO), where
 * it removes the whole shadow-ray test of every lit pixel.
 */
DEV bool plane_points_away(NodeP N, D3 from, D3 raw)
{
    const uint32_t fl = N->flags;
    double oy = (fl & kNodeZeroOffset) ? from.y : from.y - N->off[1];
    if (!(fl & kNodeIdentityMatrix)) { /* mulvm(o - off, inv).y, literally */
        const double ox = (fl & kNodeZeroOffset) ? from.x : from.x - N->off[0];
        const double oz = (fl & kNodeZeroOffset) ? from.z : from.z - N->off[2];
        oy = ox * N->inv[1] + oy * N->inv[4] + oz * N->inv[7];
    }
    const double y = N->g.p[0];
    const bool sane = (fabs(raw.x) < 1e150) & (fabs(raw.z) < 1e150);
    const bool up = (raw.y > 1e-150) & (raw.y < 1e150), down = (raw.y < -1e-150) & (raw.y > -1e150);
    return sane & (((oy > y) & up) | ((oy < y) & down));
}

/* PO (a template argument of everything from render_tile down): what the launcher knows about the scene.
 * kSpecPlanes: every node is an axis plane (plane_points_away).  kSpecIdentity: every node's matrix is the identity
 * (translations allowed) — true of every scene the reference ships; the instances compiled for it carry none of
 * Node.intersect's matrix products, no un-normalised copy of the direction through the node loops and no
 * transform in hit_surface: 124 VGPRs for both copies of the depth-1 trace instead of 128 + 24 spilled. */
enum { kSpecPlanes = 1, kSpecIdentity = 2 };

/* finish_uv: Sphere.intersect's u,v — rt/geometry.d:118-120.  `PI` is an 80-bit real there: the two expressions
 * are evaluated with the x87's 64-bit significand and rounded to double on assignment; x87.h
 * reproduces that with integer arithmetic (a NaN / infinite operand takes the plain double
 * expression, whose result is the same NaN).
 *
 * UVWant (wave-uniform): which u,v the caller of hit_surface reads.  kUVExact: those doubles — the probe, the hit
 * planes and ray queries (which report them), Checker and Procedure2 textures.  kUVBitmap: the only reader is
 * BitmapTexture.getTexColor with scaling `s`, which converts (u*s - floor(u*s)) to float at once; u,v are then
 * doubles that give THAT float bit for bit (c2_sphere_uv_bitmap, f32_certain.h) and may differ from the exact ones
 * by 2^-51.  Planes and cubes return the same u,v in both modes. */
enum { kUVNone = 0, kUVExact = 1, kUVBitmap = 2 };
struct UVWant {
    int kind;
    double s;
};
DEV UVWant uv_want(bool exact) { return UVWant{exact ? kUVExact : kUVNone, 0.0}; }

DEV void sphere_uv(double dx, double dz, double w, UVWant want, double &u, double &v)
{
    /* c2rt_trace_common.inc: real calls */
    const UV r = want.kind == kUVBitmap ? c2_sphere_uv_bitmap(dx, dz, w, want.s) : c2_sphere_uv(dx, dz, w);
    u = r.u;
    v = r.v;
}

/* ------------------------------------------------------------------ */
/* textures — rt/texture.d, rt/bitmap.d                                  */
/* ------------------------------------------------------------------ */

/* Bitmap.getFilteredPixel — rt/bitmap.d:48-63 */
DEV F3 bitmap_filtered(const float4 *texels, uint32_t width, uint32_t height, float x, float y)
{
    /* isInvalidPos(cast(size_t)x, cast(size_t)y): x, y are >= 0 or NaN here */
    if (!(x < (float)width) | !(y < (float)height) | (width == 0) | (height == 0))
        return mkf(1.0f, 0.0f, 0.0f); /* NamedColors.red */
    const float fx = floorf(x), fy = floorf(y);
    const uint32_t tx = (uint32_t)fx, ty = (uint32_t)fy;
    const uint32_t txn = tx + 1 == width ? 0 : tx + 1;
    const uint32_t tyn = ty + 1 == height ? 0 : ty + 1;
    const float p = x - fx, q = y - fy;
    const float4 c00 = texels[(size_t)ty * width + tx], c10 = texels[(size_t)ty * width + txn];
    const float4 c01 = texels[(size_t)tyn * width + tx], c11 = texels[(size_t)tyn * width + txn];
    const float w00 = (1.0f - p) * (1.0f - q), w10 = p * (1.0f - q), w01 = (1.0f - p) * q, w11 = p * q;
    return mkf(c00.x, c00.y, c00.z) * w00 + mkf(c10.x, c10.y, c10.z) * w10 + mkf(c01.x, c01.y, c01.z) * w01 +
           mkf(c11.x, c11.y, c11.z) * w11;
}

/* The same function for lean::ground_tile_certain (c2rt_trace.inc), where the bitmap is wave-uniform: `pool` is the
 * texel pool (RenderParams::texels), `offset` the bitmap's first texel in it.  Same test, floors, wraps, weights and
 * sum order — the same IEEE operations on the same operands, hence the same bits (tests/tap_average_check.hip holds it
 * to bitmap_filtered) —, with the instructions around them cut down:
 *   addresses are 32-bit byte offsets from the scalar pool pointer (global_load_dwordx3 v, v_off, s[base:base+1]).
 *     The caller guarantees offset + width * height <= 2^28 texels and width, height < 2^24 (scene_plan.cpp,
 *     fill_params, leaves a frame outside that on ground_tile): ty * width + offset is then one 24-bit multiply-add,
 *     the row below is that plus width, or `offset` itself where ty + 1 wraps, and a texel index times 16 fits 32 bits;
 *   the blend is written on (r, g) pairs as they were loaded, the weights broadcast (op_sel), and on b and the weights
 *     as single floats: a packed instruction costs 1.67 single ones on this chip, so a pair pays only without the
 *     moves that gather it (scripts/ubench/pk_f32_issue.hip, profiles/r11_variants.md). */
/* an empty asm on a product: the SLP vectoriser cannot gather it into a register pair, which it does with moves */
DEV float alone(float v)
{
    asm("" : "+v"(v));
    return v;
}
DEV F3 bitmap_filtered_uniform(const float *pool, uint32_t offset, uint32_t width, uint32_t height, float x, float y)
{
    if (!(x < (float)width) | !(y < (float)height) | (width == 0) | (height == 0))
        return mkf(1.0f, 0.0f, 0.0f); /* NamedColors.red */
    typedef float __attribute__((ext_vector_type(2))) f2_t;
    typedef float __attribute__((ext_vector_type(3))) f3_t;
    const float fx = floorf(x), fy = floorf(y);
    const uint32_t tx = (uint32_t)fx, ty = (uint32_t)fy;
    const uint32_t txn = tx + 1 == width ? 0 : tx + 1;
    const float p = x - fx, q = y - fy;
    const uint32_t row0 = __umul24(ty, width) + offset;
    const uint32_t row1 = ty + 1 == height ? offset : row0 + width;
    const char __attribute__((address_space(1))) *base = (const char __attribute__((address_space(1))) *)pool;
#define C2RT_TEXEL(i) (*(const f3_t __attribute__((address_space(1))) *)(base + (uint64_t)(uint32_t)((i) << 4)))
    const f3_t c00 = C2RT_TEXEL(row0 + tx), c10 = C2RT_TEXEL(row0 + txn);
    const f3_t c01 = C2RT_TEXEL(row1 + tx), c11 = C2RT_TEXEL(row1 + txn);
#undef C2RT_TEXEL
    const float w00 = alone((1.0f - p) * (1.0f - q)), w10 = alone(p * (1.0f - q)), w01 = alone((1.0f - p) * q), w11 = alone(p * q);
    const float b = ((alone(c00.z * w00) + alone(c10.z * w10)) + alone(c01.z * w01)) + alone(c11.z * w11);
    const f2_t rg = ((c00.xy * w00 + c10.xy * w10) + c01.xy * w01) + c11.xy * w11;
    return mkf(rg.x, rg.y, b);
}

/* A node's shading inputs in registers (DevMat, c2rt_device.h). */
struct Mat {
    int shader_type, tex_type, tex;
    float strength;
    F3 color;
    double exponent;
    uint32_t td[8];
};

/* a node's shading inputs, from its record (wave-uniform address: scalar loads) */
DEV void load_mat(NodeP N, Mat &m)
{
    MatP M = &N->mat;
    m.shader_type = M->shader_type;
    m.tex_type = M->tex_type;
    m.tex = M->tex;
    m.strength = M->strength;
    m.color = ldf3(M->color);
    m.exponent = M->exponent;
#pragma unroll
    for (int i = 0; i < 8; ++i) m.td[i] = M->texdata[i];
}

/* Checker.getTexColor — rt/texture.d:36-54 */
DEV F3 checker_color(const Mat &m, double u, double v)
{
    const double size = __hiloint2double((int)m.td[7], (int)m.td[6]);
    const int x = d2i_x86(floor(u / size));
    const int y = d2i_x86(floor(v / size));
    const int white = (int)((uint32_t)x + (uint32_t)y) % 2;
    return white ? mkf(__uint_as_float(m.td[3]), __uint_as_float(m.td[4]), __uint_as_float(m.td[5]))
                 : mkf(__uint_as_float(m.td[0]), __uint_as_float(m.td[1]), __uint_as_float(m.td[2]));
}

/* BitmapTexture.getTexColor — rt/texture.d:116-126 */
DEV F3 bitmap_color(const RenderParams &P, const Mat &m, double u, double v)
{
    const double s = (double)__uint_as_float(m.td[2]);
    u *= s;
    v *= s;
    u = u - floor(u);
    v = v - floor(v);
    const uint32_t w = m.td[0], hgt = m.td[1];
    const float tx = (float)u * (float)w;
    const float ty = (float)v * (float)hgt;
    const uint64_t offset = (uint64_t)m.td[4] | ((uint64_t)m.td[5] << 32);
    return bitmap_filtered(reinterpret_cast<const float4 *>(P.texels) + offset, w, hgt, tx, ty);
}

DEV F3 tex_color(const RenderParams &P, const Mat &m, double u, double v)
{
    const int type = m.tex_type;
    if (type == C2RT_TEX_CHECKER) {
        return checker_color(m, u, v);
    } else if (type == C2RT_TEX_PROCEDURE2) { /* Procedure2.getTexColor — rt/texture.d:77-86 */
        TexP T = (TexP)P.textures + m.tex;
        F3 result = mkf(0, 0, 0);
#pragma unroll
        for (int i = 0; i < 3; ++i)
            result = result + (ldf3(T->color + 3 * i) * (float)c2_sin(u * T->param[i]) +
                               ldf3(T->color + 9 + 3 * i) * (float)c2_sin(v * T->param[3 + i]));
        return result;
    } else {
        return bitmap_color(P, m, u, v);
    }
}

/* Counter-based RNG for the lens samples (build-defined: the reference draws from libc rand(),
 * util/random.d:19-28, which is not reproducible — SURVEY.md F5).  32-bit multiply-xorshift
 * finaliser ("lowbias32"); the key folds (seed, pixel, tap) once per sample loop, a draw is one
 * hash of key + golden-ratio * counter.  The CPU checker restates it statement for statement. */
DEV uint32_t hash32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
DEV uint32_t rng_key(uint64_t seed, uint64_t pixel, uint32_t tap)
{
    uint32_t k = hash32((uint32_t)(seed >> 32) ^ 0x243f6a88u);
    k = hash32(k ^ (uint32_t)seed);
    k = hash32(k + (uint32_t)(pixel >> 32));
    k = hash32(k ^ (uint32_t)pixel);
    return hash32(k + tap);
}
/* uniform in [0, 1) with 32 random bits (rand()/RAND_MAX has 31) */
DEV double rng_uniform(uint32_t key, uint32_t sample, uint32_t dim)
{
    return (double)hash32(key + 0x9e3779b9u * (sample * 16u + dim + 1u)) * 0x1p-32;
}

struct Rng { uint32_t key, sample, dim; };
DEV double rng_next(Rng &r) { return rng_uniform(r.key, r.sample, r.dim++); }

/* (sin, cos)(2 pi u) for u in [0, 1) without libm, so that a CPU checker and the kernel produce the
 * same bits (device sincos and glibc sin/cos differ by an ulp, which flips z-fights between
 * coincident planes): exact reduction of 4u to a quadrant q and a fraction g in [0, 0.5] (mirrored
 * about the octant boundary), then the Taylor polynomials in theta = g * (pi/2) <= pi/4 — sin to
 * theta^17, cos to theta^16, truncation error < 1e-17 — evaluated by Horner in fp64 with contraction
 * off (integer and IEEE +, * only: any IEEE-754 host reproduces it). */
DEV void lens_sincos2pi(double u, double &sn, double &cs)
{
    const double t = u * 4.0;          /* exact */
    const int q = (int)t;              /* 0..3 */
    const double f = t - (double)q;    /* exact, [0, 1) */
    const bool mirror = f > 0.5;
    const double g = mirror ? 1.0 - f : f; /* exact */
    const double th = g * 0x1.921fb54442d18p+0; /* pi/2 */
    const double z = th * th;
    double ps = 0x1.952c77030ad4ap-49;             /* +1/17! */
    ps = -0x1.ae7f3e733b81fp-41 + z * ps;          /* -1/15! */
    ps = 0x1.6124613a86d09p-33 + z * ps;           /* +1/13! */
    ps = -0x1.ae64567f544e4p-26 + z * ps;          /* -1/11! */
    ps = 0x1.71de3a556c734p-19 + z * ps;           /* +1/9! */
    ps = -0x1.a01a01a01a01ap-13 + z * ps;          /* -1/7! */
    ps = 0x1.1111111111111p-7 + z * ps;            /* +1/5! */
    ps = -0x1.5555555555555p-3 + z * ps;           /* -1/3! */
    const double s = th + th * (z * ps);
    double pc = 0x1.ae7f3e733b81fp-45;             /* +1/16! */
    pc = -0x1.93974a8c07c9dp-37 + z * pc;          /* -1/14! */
    pc = 0x1.1eed8eff8d898p-29 + z * pc;           /* +1/12! */
    pc = -0x1.27e4fb7789f5cp-22 + z * pc;          /* -1/10! */
    pc = 0x1.a01a01a01a01ap-16 + z * pc;           /* +1/8! */
    pc = -0x1.6c16c16c16c17p-10 + z * pc;          /* -1/6! */
    pc = 0x1.5555555555555p-5 + z * pc;            /* +1/4! */
    pc = -0.5 + z * pc;                            /* -1/2! */
    const double c = 1.0 + z * pc;
    const double a = mirror ? c : s, b = mirror ? s : c; /* sin, cos of the in-quadrant angle */
    /* quadrant rotation: q=0 (a, b), 1 (b, -a), 2 (-a, -b), 3 (-b, a) */
    sn = (q & 1) ? b : a;
    cs = (q & 1) ? a : b;
    if (q == 2 || q == 3) sn = -sn;
    if (q == 1 || q == 2) cs = -cs;
}

/* rays a lane traced (raytrace, shade; read by the counting instances only: render_tile's CNT) */
struct Counters { uint32_t primary, shadow; };

/* adjustSaturation + combineStereo — rt/color.d:10-15,77-83 */
DEV F3 desaturate(F3 c, float amount)
{
    const float mid = (c.r + c.g + c.b) / 3;
    return mkf(c.r * amount + mid * (1 - amount), c.g * amount + mid * (1 - amount), c.b * amount + mid * (1 - amount));
}
DEV F3 combine_stereo(F3 l, F3 r)
{
    l = desaturate(l, 0.25f);
    r = desaturate(r, 0.25f);
    return l * mkf(1, 0, 0) + r * mkf(0, 1, 1);
}

/* Two steps of render_tile for ground_tile.  (render_tile keeps its own lines: taking them from here reorders
 * instructions in instances that have no ground path, and those are to stay what every measurement was taken on.) */
/* local row -> frame row under interleaved strips */
DEV uint32_t frame_row(const RenderParams &P, const uint32_t lr)
{
    uint32_t y = lr;
    if (P.strip_world > 1) {
        const uint32_t sh = P.strip_height;
        y = ((lr / sh) * P.strip_world + P.strip_rank) * sh + lr % sh;
    }
    return y;
}

/* a finished pixel, float RGB or display-encoded */
DEV void store_pixel(const RenderParams &P, const size_t pixel_index, const F3 accum)
{
    if (P.out_rgb32) { /* wave-uniform */
        /* Color.toRGB32 via convertTo8bit_sRGB_Cached (rt/color.d:154-162,209-214), fused: the display frame
         * needs neither a float frame in HBM nor a second kernel (c2rt_render_frame_rgb32) */
        const float c3[3] = {accum.r, accum.g, accum.b};
        uint32_t ch[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) ch[c] = !(c3[c] > 0) ? 0u : (c3[c] >= 1 ? 255u : (uint32_t)P.srgb_lut[(int)(c3[c] * 4096.0f)]);
        P.out_rgb32[pixel_index] = ch[2] | (ch[1] << 8) | (ch[0] << 16);
    } else {
        /* one 12-byte store per lane (global_store_dwordx3): 8 lanes cover a tile row's 96 contiguous bytes */
        typedef float __attribute__((ext_vector_type(3), aligned(4))) f3_t;
        f3_t v3;
        v3.x = accum.r;
        v3.y = accum.g;
        v3.z = accum.b;
        *reinterpret_cast<f3_t *>(P.out + pixel_index * 3) = v3;
    }
}

/* accum / n for ground_tile_certain: `Color / float` (rt/color.d:128-132) through the lean fp32 quotient of fp64_lean.h,
 * the refined reciprocal of the wave-uniform tap count taken once.  Every channel must be +0 — a sky pixel, a black
 * texel: +0 * r, the two remainders and the two sums are all +0, as +0 / n is — or a positive float in [2^-60, 2^60),
 * where the sequence is the compiler's division bit for bit (tests/tap_average_check.hip); any other channel is noted in
 * `bad` like an operand outside a lean window, and the tile is rendered by ground_tile, which divides the long way.  That
 * includes every negative channel, -0 among them (the sequence would return +0 for it): no floor the reference can
 * describe has one.
 * v = bits - bits(2^-60) is below bits(2^60) - bits(2^-60) exactly for those positive floats, +0 is let through as
 * v = 0, and half the largest v of the three is on the accumulator's scale. */
DEV void tap_average(Oob &bad, F3 &accum, const float n)
{
    constexpr uint32_t kLo = (uint32_t)(127 - 60) << 23, kSpan = (uint32_t)120 << 23;
    static_assert((kSpan >> 1) == ((uint32_t)(kWinHi - kWinLo) << kOobShift), "oob_any's threshold");
    const uint32_t br = __float_as_uint(accum.r), bg = __float_as_uint(accum.g), bb = __float_as_uint(accum.b);
    const uint32_t vr = br == 0u ? 0u : br - kLo, vg = bg == 0u ? 0u : bg - kLo, vb = bb == 0u ? 0u : bb - kLo;
    const uint32_t vrg = vr > vg ? vr : vg, v = vrg > vb ? vrg : vb;
    const uint32_t t = v >> 1;
    bad.t = bad.t > t ? bad.t : t;
    const float rn = rcp_refined_f32(n);
    accum = mkf(div_with_f32(accum.r, n, rn), div_with_f32(accum.g, n, rn), div_with_f32(accum.b, n, rn));
}

/* what ground_tile (c2rt_trace.inc) returns */
enum { kGroundDone = 0, kGroundRedo = 1, kGroundBail = 2 };

/*
 * c2rt.h — plain-C boundary of the MI355X render hot path for Chess2RT.
 *
 * The reference (D) has no FFI of its own; the seam this
 * library plugs into is the body of the render-thread lambda in
 * `rt/renderer.d:36-37` (`Renderer(scene, output, ..).renderRT()`) and the
 * pixel probe `renderPixel` (`rt/renderer.d:46-57`).  The D side keeps its
 * `Scene` / `Camera` / `Renderer` API; it flattens the scene into the tables
 * below once per scene load (`c2rt_upload_scene`), calls
 * `scene.beginFrame()` itself (`rt/scene.d:55-58`, `rt/camera.d:77-117`) and
 * hands the six camera vectors over per frame (`c2rt_render_frame`).
 *
 * Conventions
 *   - every function returns a `c2rt_status`; nothing throws across the ABI;
 *   - all tables are COPIED at call time (the D GC may move/free its data);
 *   - geometry is fp64, colour is fp32, exactly as in the reference
 *     (`rt/imported_types.d:10-11`, `rt/color.d:27-35`);
 *   - matrices are the 9 doubles of gfm `mat3d` in row-major order `c[i][j]`,
 *     used as ROW-vector x matrix (`rt/imported_types.d:13-20`);
 *   - the frame is `Image!Color`: W*H*3 float32, row-major, no padding
 *     (`imageio/image.d:18-54`).
 *   - one context per process and GPU; calls on a context are serialised by
 *     the caller (the reference has a single render thread).
 *
 * Environment: the product library (libc2rt.so) reads NO environment variable.
 * The measurement / test knobs (C2RT_EXACT, C2RT_HOST_DIRECT_STORE,
 * C2RT_CSG_FIRST_CAP, C2RT_DEBUG_CULL — none changes a pixel) exist only in the
 * diagnostics build, chess2rt_amd/libc2rt_diag.so (`make`: c2rt_api.cpp with
 * -DC2RT_DIAG=1 over the same kernel objects), where each is read once per
 * process; chess2rt_amd/csrc/c2rt_api.cpp documents them at their sites.
 */
#ifndef C2RT_H
#define C2RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C2RT_ABI_VERSION 1u

/* hard limits of the device path (upload fails with C2RT_ERR_LIMIT beyond) */
#define C2RT_MAX_CSG_DEPTH 4   /* nesting levels of CsgOp under a node       */
#define C2RT_MAX_CSG_GEOMS 4096 /* geometries in a scene that has CsgOps (hit lists tag leaves in 12 bits) */
#define C2RT_MAX_CSG_HITS 8    /* hits kept per CSG child per ray (the reference
                                  grows a MyArray, util/array.d:54-63; a sane
                                  primitive yields at most 2)                 */

typedef enum c2rt_status {
    C2RT_OK = 0,
    C2RT_ERR_INVALID_ARG = 1,   /* null pointer, bad index, bad enum          */
    C2RT_ERR_NO_DEVICE = 2,     /* no gfx950 GPU / HIP runtime failure        */
    C2RT_ERR_HIP = 3,           /* a HIP call failed; see c2rt_last_error     */
    C2RT_ERR_UNSUPPORTED = 4,   /* GIEnabled, unknown entity type, ...        */
    C2RT_ERR_LIMIT = 5,         /* CSG depth, sizes beyond the device limits  */
    C2RT_ERR_NO_SCENE = 6,      /* render before upload                       */
    C2RT_ERR_CANCELLED = 7,     /* stop flag was raised between passes        */
    C2RT_ERR_IO = 8,            /* host loader: file missing / unreadable     */
    C2RT_ERR_PARSE = 9          /* host loader: invalid scene / image file    */
} c2rt_status;

/* Closed type sets of the reference. */
typedef enum c2rt_geom_type {      /* rt/geometry.d:15,73,149,357,367,377 */
    C2RT_GEOM_PLANE = 0,
    C2RT_GEOM_SPHERE = 1,
    C2RT_GEOM_CUBE = 2,
    C2RT_GEOM_CSG_UNION = 3,
    C2RT_GEOM_CSG_INTER = 4,
    C2RT_GEOM_CSG_DIFF = 5
} c2rt_geom_type;

typedef enum c2rt_shader_type {    /* rt/shader.d:54,177 */
    C2RT_SHADER_LAMBERT = 0,
    C2RT_SHADER_PHONG = 1
} c2rt_shader_type;

typedef enum c2rt_texture_type {   /* rt/texture.d:20,70,103 */
    C2RT_TEX_CHECKER = 0,
    C2RT_TEX_PROCEDURE2 = 1,
    C2RT_TEX_BITMAP = 2
} c2rt_texture_type;

typedef enum c2rt_light_type {     /* rt/light.d:52 */
    C2RT_LIGHT_POINT = 0
} c2rt_light_type;

/*
 * Flat scene: struct-of-arrays tables, indices instead of references.
 * Replaces the object graph reached from `Scene` (rt/scene.d:39-53).
 */
typedef struct c2rt_scene_desc {
    uint32_t abi_version;          /* = C2RT_ABI_VERSION */

    /* ---- geometries (Scene.geometries, rt/geometry.d) ------------------ */
    uint32_t n_geoms;
    const int32_t *geom_type;      /* [n_geoms] c2rt_geom_type */
    /* [n_geoms][4] doubles:
     *   plane : y, limit (NaN = unbounded, rt/geometry.d:18-23), -, -
     *   sphere: center.x, center.y, center.z, R          (rt/geometry.d:75-79)
     *   cube  : center.x, center.y, center.z, side       (rt/geometry.d:151-152)
     *   csg   : unused */
    const double *geom_param;
    /* [n_geoms][2] left,right geometry index for CSG (rt/geometry.d:253-257),
     * -1 otherwise.  Children must have a smaller index than their parent
     * is NOT required; cycles are rejected. */
    const int32_t *geom_child;

    /* ---- textures (Scene.textures, rt/texture.d) ----------------------- */
    uint32_t n_textures;
    const int32_t *tex_type;       /* [n_textures] c2rt_texture_type */
    /* [n_textures][18] floats:
     *   checker   : color1.rgb, color2.rgb                 (rt/texture.d:22)
     *   procedure2: colorU[0..3].rgb, colorV[0..3].rgb     (rt/texture.d:72)
     *   bitmap    : unused */
    const float *tex_color;
    /* [n_textures][6] doubles:
     *   checker   : size                                   (rt/texture.d:23)
     *   procedure2: freqU[0..3], freqV[0..3]               (rt/texture.d:73)
     *   bitmap    : unused */
    const double *tex_param;
    const float *tex_scaling;      /* [n_textures] BitmapTexture.scaling (rt/texture.d:155) */
    const uint32_t *tex_width;     /* [n_textures] bitmap width  (0 if not a bitmap) */
    const uint32_t *tex_height;    /* [n_textures] bitmap height */
    const uint64_t *tex_offset;    /* [n_textures] first texel of this bitmap in `texels` */
    /* texel pool: linear-RGB float triples, row-major, y = 0 is the TOP row,
     * already gamma-decoded (rt/bitmap.d:116-136) — i.e. Bitmap.data.pixels. */
    uint64_t n_texels;
    const float *texels;           /* [n_texels][3] */

    /* ---- shaders (Scene.shaders, rt/shader.d) -------------------------- */
    uint32_t n_shaders;
    const int32_t *shader_type;    /* [n_shaders] c2rt_shader_type */
    const float *shader_color;     /* [n_shaders][3] Shader.color (rt/shader.d:26) */
    const int32_t *shader_texture; /* [n_shaders] texture index or -1 */
    const double *shader_exponent; /* [n_shaders] Phong.exponent (rt/shader.d:180) */
    const float *shader_strength;  /* [n_shaders] Phong.strength (rt/shader.d:181) */

    /* ---- lights (Scene.lights, rt/light.d) ----------------------------- */
    uint32_t n_lights;
    const int32_t *light_type;     /* [n_lights] c2rt_light_type */
    const double *light_pos;       /* [n_lights][3] PointLight.pos */
    const float *light_color;      /* [n_lights][3] Light.lightColor */
    const float *light_power;      /* [n_lights]    Light.lightPower */

    /* ---- nodes (Scene.nodes, rt/node.d:7-10, rt/transform.d:11-14) ----- */
    uint32_t n_nodes;
    const int32_t *node_geom;      /* [n_nodes] geometry index */
    const int32_t *node_shader;    /* [n_nodes] shader index */
    const int32_t *node_bump;      /* [n_nodes] texture index or -1 (base modifyNormal is a no-op) */
    /* [n_nodes][30] doubles: transform[9], inverseTransform[9],
     * transposedInverse[9], offset[3] */
    const double *node_transform;

    /* ---- the GlobalSettings fields the path reads (rt/global_settings.d) */
    float ambient[3];              /* ambientLightColor */
    uint32_t max_trace_depth;      /* maxTraceDepth (primary rays have depth 0) */
    uint32_t gi_enabled;           /* GIEnabled: must be 0 (C2RT_ERR_UNSUPPORTED otherwise) */
} c2rt_scene_desc;

/*
 * Per-frame camera state = what `Camera.beginFrame` leaves behind
 * (rt/camera.d:47-53,77-117) plus the fields `getScreenRay` reads
 * (rt/camera.d:123-173).
 */
typedef struct c2rt_camera_frame {
    double pos[3];
    double up_left[3], up_right[3], down_left[3];
    double right_dir[3], up_dir[3], front_dir[3];
    double frame_width, frame_height;   /* Camera.frameWidth/Height as doubles */
    /* depth of field (rt/camera.d:41-44,154-173); dof==0 for parity runs */
    uint32_t dof;
    uint32_t num_samples;               /* Camera.numSamples (default 25) */
    double focal_plane_dist;
    double disc_multiplier;             /* 10 / fNumber */
    double stereo_separation;           /* 0 = mono (rt/renderer.d:305) */
} c2rt_camera_frame;

/* Sampling modes (SURVEY.md F6, section 8(d) "spp mapping"). */
typedef enum c2rt_tap_mode {
    C2RT_TAPS_1 = 1,      /* AAEnabled=false: one sample at (x, y)            */
    C2RT_TAPS_REF5 = 5,   /* AAEnabled=true: reference 5-tap table, sum / 5   */
    C2RT_TAPS_4 = 4       /* build-defined "4 spp": the first four entries of the table, (0, 0) included, sum / 4 */
} c2rt_tap_mode;

typedef struct c2rt_render_opts {
    uint32_t width, height;        /* settings.frameWidth / frameHeight = output size */
    uint32_t taps;                 /* c2rt_tap_mode */
    /* Interleaved row-strip sharding (multi-GPU): this call renders strips
     * s = strip_rank, strip_rank + strip_world, ... of height strip_height
     * into a compact buffer of those strips only.  strip_world <= 1 renders
     * the whole frame. */
    uint32_t strip_height;
    uint32_t strip_rank;
    uint32_t strip_world;
    uint64_t seed;                 /* counter-based RNG seed (DOF only) */
    uint32_t count_rays;           /* 1: also count primary/shadow rays cast */
    /* 0: the normal frame.  N > 0: `prepassOnly` (rt/renderer.d:110-130) with
     * bucketSize N: every 16x16 block of every NxN bucket is filled with the one
     * sample taken at its top-left pixel (with depth of field its jitter spans
     * the clipped block, rt/renderer.d:119,277); taps are ignored (the
     * reference returns before the AA pass). */
    uint32_t prepass_bucket;
} c2rt_render_opts;

/* What `renderPixel` returns (TraceResult, rt/renderer.d:15-21). */
typedef struct c2rt_trace_result {
    float color[3];
    int32_t closest_node;          /* -1: no hit */
    int32_t leaf_geom;             /* IntersectionData.g (leaf geometry index) */
    double p[3], normal[3];
    double dist, u, v;
    double ray_orig[3], ray_dir[3];
} c2rt_trace_result;

typedef struct c2rt_ray_stats {
    uint64_t primary_rays;
    uint64_t shadow_rays;
} c2rt_ray_stats;

typedef struct c2rt_ctx c2rt_ctx;

/* ---- lifecycle ---------------------------------------------------------- */

/* device < 0: use the current HIP device.  Fails with C2RT_ERR_NO_DEVICE when
 * no GPU is visible: there is NO CPU fallback in this library. */
int c2rt_init(int device, c2rt_ctx **out);

/* ONE context over several GPUs of this process — SURVEY.md 8(b)'s
 * `c2rt_init(int device_count_or_0, ...)`: what a single-process host like the
 * reference (one render thread fanning out, rt/renderer.d:23-44,133-142) needs
 * to use a whole node.  device_count_or_0 = 0 opens every visible GPU;
 * `device_ids` (nullable) names the HIP device of each slot — entries may
 * repeat, which runs several slots on one GPU (how a 1-GPU box exercises this
 * path).  Slot 0 is the lead device.  On such a context
 *   - c2rt_upload_scene replicates the tables on every device;
 *   - c2rt_render_frame / c2rt_render_frame_rgb32 deal interleaved 8-row strips
 *     to the devices (opts->strip_world must be <= 1) and every device copies
 *     its finished strips straight into the caller's host frame over its own
 *     PCIe link (strided 2-D copies; pin the buffer with c2rt_pin_host_buffer);
 *   - c2rt_render_frame_device: `out_rgb_dev` lives on the lead device and the
 *     other devices' kernels store their strips straight into it over xGMI
 *     (peer access) — no gather buffer, no de-interleave pass;
 *   - c2rt_render_pixel and the strip / encode helpers run on the lead device.
 * C2RT_ERR_NO_DEVICE when a device id is out of range; C2RT_ERR_UNSUPPORTED
 * from c2rt_render_frame_device when a device cannot peer-map the lead.
 * EXPERIMENTAL on more than one PHYSICAL device: the GPU pool this was built
 * on shows a job one GPU, so every test runs the slots on one device (ids
 * repeated); peer access, cross-device events and the parallel copies have
 * not executed across two GPUs yet.  A failing slot leaves the lead device
 * current and the caller's stream ordered after every slot already launched. */
int c2rt_init_multi(int device_count_or_0, const int *device_ids, c2rt_ctx **out);
/* number of device slots of the context (1 for c2rt_init) */
int c2rt_device_count(const c2rt_ctx *ctx);
void c2rt_destroy(c2rt_ctx *ctx);
const char *c2rt_last_error(const c2rt_ctx *ctx);
const char *c2rt_status_string(int status);
uint32_t c2rt_abi_version(void);

/* ---- scene -------------------------------------------------------------- */

/* Validates and copies the tables into HBM.  Replaces the implicit "scene is
 * GC memory shared with the render thread" of rt/renderer.d:39-40. */
int c2rt_upload_scene(c2rt_ctx *ctx, const c2rt_scene_desc *scene);
/* Identity of the tables the context holds now: a process-wide counter value
 * assigned by each successful c2rt_upload_scene (never reused, never 0; 0 = no
 * scene).  A host-side scene object remembers the value of ITS upload and
 * re-uploads when the context has moved on to another scene. */
uint64_t c2rt_scene_generation(const c2rt_ctx *ctx);

/* ---- posing the uploaded scene: node transforms and lights ---------------- */

/* New values for some node transforms and lights of the uploaded scene.  Everything else of the description —
 * geometries, shaders, textures, texels, the counts — is what was uploaded; changing those is a re-upload. */
typedef struct c2rt_scene_pose {
    uint32_t n_nodes;              /* entries below; 0: no node changes */
    const uint32_t *node_index;    /* [n_nodes] indices into the uploaded scene's nodes */
    /* [n_nodes][30], the layout of c2rt_scene_desc::node_transform: transform[9], inverseTransform[9],
     * transposedInverse[9], offset[3].  All four parts are the caller's, as at upload: the library never inverts a
     * matrix, the inverse's bits are those of the caller's own Transform (rt/transform.d:24-55). */
    const double   *node_transform;
    uint32_t n_lights;
    const uint32_t *light_index;   /* [n_lights] */
    const double   *light_pos;     /* [n_lights][3], nullable: positions unchanged */
    const float    *light_color;   /* [n_lights][3], nullable */
    const float    *light_power;   /* [n_lights],   nullable */
} c2rt_scene_pose;

/* Patches the uploaded scene in place.  Afterwards the context behaves, in every entry point and in every bit, as if
 * c2rt_upload_scene had been called with the uploaded description patched by `pose`: the library keeps a copy of that
 * description (without the texels), patches it, plans it again on the host — which instance a frame runs, the ground
 * plane, the shadow rectangles, the candidates of the mask pre-pass all follow — and copies to the device the node
 * records, the light table and the shadow rectangles whose bytes changed.  Poses accumulate: each update patches the
 * scene the one before it left.
 *
 * c2rt_scene_generation does NOT change: it names the upload, and this is the same description posed differently.  A
 * host-side scene object that moved its own node keeps its generation and needs no re-upload.
 *
 * Ordering.  The table copies are stream-ordered copies from pageable host memory on `hip_stream` (a hipStream_t,
 * NULL = default stream): the runtime has read their source when the call returns, and they run after everything
 * enqueued earlier on that stream.  Frames, batches and queries enqueued on `hip_stream` BEFORE the call see the old
 * scene, those enqueued AFTER it the new one, with no host sync in between.  The host-side plan changes when the call
 * returns.  Work of this context on OTHER streams is not ordered against the update by the library: a frame still
 * running there may read either table — the caller's hazard, like two frames into one buffer.  The call may wait, on the
 * host, until work enqueued earlier on `hip_stream` has drained (as c2rt_render_frames_device may); it never waits for
 * other streams, synchronises the device, allocates, frees, records or waits for an event, touches the texel pool,
 * or keeps `hip_stream`.  With `hip_stream` NULL the call also waits, on the host, for its own copies on the default
 * stream: the host-output entry points (c2rt_render_frame, c2rt_render_frames, the queries) run on the context's own
 * stream, which is not ordered behind the default stream, and must see the new scene when the call has returned.
 *
 * Statuses, all decided before anything is enqueued or changed — a refused update leaves the scene exactly as it was
 * (unlike c2rt_upload_scene): no scene: C2RT_ERR_NO_SCENE; C2RT_ERR_INVALID_ARG for a null `pose`, a count > 0 with a
 * null index array, n_nodes > 0 with a null node_transform, n_lights > 0 with all three light arrays null, an index
 * out of range or listed twice (c2rt_last_error names the entry); whatever the scene planner answers to the patched
 * description, with its message.  A pose with both counts 0 is C2RT_OK and enqueues nothing.
 *
 * A context of c2rt_init_multi patches every device slot; `hip_stream` must be NULL there (C2RT_ERR_INVALID_ARG
 * otherwise).  Each further slot's copies are ordered on that slot's own stream, as its frames are; the lead slot's
 * go to the default stream and are waited for, as above. */
int c2rt_update_scene(c2rt_ctx *ctx, const c2rt_scene_pose *pose, void *hip_stream);

/* ---- rendering ---------------------------------------------------------- */

/* Number of rows this rank renders under `opts` striping (== opts->height
 * when strip_world <= 1). */
uint32_t c2rt_local_rows(const c2rt_render_opts *opts);

/* Blocking frame render into caller-owned HOST memory (`Image!Color.pixels`):
 * the drop-in for `Renderer.renderRT()` (rt/renderer.d:83-192).  Writes
 * local_rows*width*3 floats.  `stop_flag` (nullable) is polled like
 * `isStopReq()` (rt/renderer.d:93-97,129,147,180): before the frame and, for a
 * frame that goes back in row chunks (a page-locked float frame), between the
 * chunks.  A frame made by ONE launch — pageable destination, or display words
 * stored straight into a page-locked frame (c2rt_render_frame_rgb32) — polls it
 * once, before the launch; C2RT_ERR_CANCELLED leaves the frame unspecified. */
int c2rt_render_frame(c2rt_ctx *ctx, const c2rt_camera_frame *cam,
                      const c2rt_render_opts *opts, float *out_rgb,
                      const volatile uint8_t *stop_flag);

/* Optional: declare a long-lived host frame buffer (the GUI's `screen`,
 * gui/raytracer_demo.d:181-182) so that c2rt_render_frame can page-lock it once
 * and stream the frame back at PCIe rate while later rows are still rendering.
 * The caller must unpin before freeing the buffer.  Without it
 * c2rt_render_frame copies into pageable memory (slower, same result). */
int c2rt_pin_host_buffer(c2rt_ctx *ctx, float *out_rgb, size_t bytes);
int c2rt_unpin_host_buffer(c2rt_ctx *ctx, float *out_rgb);

/* Same, but the output stays in HBM: `out_rgb_dev` is a device pointer
 * (e.g. a torch tensor's data_ptr) and the kernels are enqueued on
 * `hip_stream` (a hipStream_t, NULL = default stream) without a host sync.
 * Frames enqueued on one stream run in order, as everything on a HIP stream
 * does.  Frames of ONE context on DIFFERENT streams are independent of each
 * other and may overlap: the per-frame scratch a launch needs (the tile-mask
 * table, the nested-CSG retry list) exists once per stream the context has
 * rendered on (16 slots; a 17th stream recycles the least recently used one
 * after a device sync), so the call neither waits for an earlier frame nor
 * leaves an event in the queue.  The one shared resource is the ray counters:
 * frames with opts->count_rays = 1 are ordered among themselves on the device.
 * The library keeps no reference to `hip_stream` (the handle is only compared):
 * the caller may destroy it as soon as the call has returned.  The caller owns
 * the usual hazards of its buffers (two frames into one `out_rgb_dev`). */
int c2rt_render_frame_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam,
                             const c2rt_render_opts *opts, float *out_rgb_dev,
                             void *hip_stream);

/* ---- a batch of frames: many cameras, one scene, one call ----------------- */

/* Most frames one batch call takes (the per-stream table of parameter blocks
 * is 3.4 KiB per frame); C2RT_ERR_LIMIT beyond. */
#define C2RT_MAX_BATCH_FRAMES 256

/* `n_frames` frames of the uploaded scene, one per camera of `cams`, under ONE
 * set of options (same size, taps and strip assignment), with one mask
 * pre-pass launch and one frame launch for all of them (two frame launches for
 * scenes with nested CsgOps) instead of that per frame.  Frame i occupies
 * out_rgb_dev + i * local_rows * width * 3 floats and holds exactly the bits
 * c2rt_render_frame_device(ctx, &cams[i], opts, ...) writes there.  Row strips
 * (opts->strip_world > 1) work as in the single-frame call.
 *
 * Enqueued on `hip_stream` without a host sync and without leaving an event
 * in the queue, under the per-stream scratch rules of c2rt_render_frame_device
 * (the batch uses the stream's slot, with the tables multiplied): batches and
 * single frames on one stream stay ordered and may follow each other without a
 * sync; batches on different streams are independent.  When the call can
 * BLOCK: the per-frame parameter table goes to the device with a stream-ordered
 * copy from pageable memory, which the runtime stages before it returns — so
 * the call may wait, on the host, until work enqueued EARLIER on `hip_stream`
 * has drained (never for later work, never for other streams); it also blocks,
 * like every frame call, when the stream's scratch has to grow (first call,
 * more frames, a larger frame) or a 17th stream recycles a slot.  The host
 * work of the batch (culling set-up of every camera) is done before that copy.
 *
 * Statuses, all decided before anything is enqueued (the output is untouched):
 * n_frames == 0 is C2RT_OK and writes nothing (`cams` is not read); null `cams`
 * or `opts`: C2RT_ERR_INVALID_ARG; n_frames > C2RT_MAX_BATCH_FRAMES:
 * C2RT_ERR_LIMIT; C2RT_ERR_UNSUPPORTED, with c2rt_last_error naming the cause,
 * for a camera with `dof` or `stereo_separation != 0` (those kernel instances
 * carry lens state and have no batch twin), opts->count_rays (the counters
 * belong to one frame), opts->prepass_bucket, and a multi-device context.
 * All of these stay available frame by frame.  c2rt_get_exact_redos counts a
 * batch's tiles exactly as it counts single frames'. */
int c2rt_render_frames_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams,
                              uint32_t n_frames, const c2rt_render_opts *opts,
                              float *out_rgb_dev, void *hip_stream);

/* The same into HOST memory (n_frames * local_rows * width * 3 floats):
 * rendered into the context's staging buffer on the context's own stream and
 * returned with one copy; blocks until the frames are there.  `stop_flag`
 * (nullable) is polled once, before the launches: C2RT_ERR_CANCELLED then
 * leaves `out_rgb` untouched. */
int c2rt_render_frames(c2rt_ctx *ctx, const c2rt_camera_frame *cams,
                       uint32_t n_frames, const c2rt_render_opts *opts,
                       float *out_rgb, const volatile uint8_t *stop_flag);

/* An animation in one call: c2rt_render_frames_device with a pose per frame.  Frame i is the context's current scene
 * with poses[i] applied — each pose relative to the current scene, not to the frame before it — seen through cams[i],
 * and holds exactly the bits c2rt_update_scene(&poses[i]) followed by c2rt_render_frame_device(&cams[i]) writes.  A
 * pose with both counts 0 is a frame of the scene as it is.  The context's scene is unchanged by the call.
 *
 * Every frame is planned on the host like an update (instance, ground plane, shadow rectangles, pre-pass candidates,
 * culling rectangles); the node, light and rectangle tables of the frames that differ from the context's travel to
 * the device beside the batch's parameter table, in the stream's scratch slot, with the same stream-ordered copy.
 * One launch runs one kernel instance: frames whose poses leave every matrix the identity and frames whose poses do
 * not share the general instance, which the library holds to the same bits as the identity instance; a batch whose
 * poses differ in whether every node is an axis plane (the plane instances of single-light scenes) is rendered as
 * two groups of frames that agree, one launch pair per group.
 *
 * Blocking, streams and scratch: as c2rt_render_frames_device.  Statuses, all decided before anything is enqueued (the
 * output is untouched): those of c2rt_render_frames_device; null `poses` with n_frames > 0: C2RT_ERR_INVALID_ARG;
 * those of c2rt_update_scene for every poses[i], with "frame i: " in front of the message. */
int c2rt_render_frames_posed_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams,
                                    const c2rt_scene_pose *poses, uint32_t n_frames,
                                    const c2rt_render_opts *opts, float *out_rgb_dev,
                                    void *hip_stream);
/* The same into HOST memory, as c2rt_render_frames is to c2rt_render_frames_device. */
int c2rt_render_frames_posed(c2rt_ctx *ctx, const c2rt_camera_frame *cams,
                             const c2rt_scene_pose *poses, uint32_t n_frames,
                             const c2rt_render_opts *opts, float *out_rgb,
                             const volatile uint8_t *stop_flag);

/* Ray counters of the last render call made with opts->count_rays = 1
 * (waits, on the host, for that frame to complete). */
int c2rt_get_ray_stats(c2rt_ctx *ctx, c2rt_ray_stats *out);

/* CsgOp child hit lists that reached C2RT_MAX_CSG_HITS during the last render call made with
 * opts->count_rays = 1 (events, over primary and shadow rays; tiles redone by the hit-stack retry launch
 * count twice).  The reference's findAllIntersections loops `while (true)`
 * (rt/geometry.d:271-290) and does not terminate when the 1e-6 step is absorbed or a hit is NaN; this
 * build stops after C2RT_MAX_CSG_HITS hits per child (a primitive yields at most 2).  0 means the cap
 * did not take part in the frame; > 0 flags build-defined results (pathological coordinates, or a
 * nested child with more than 8 boundary crossings along one ray). */
int c2rt_get_csg_truncations(c2rt_ctx *ctx, uint64_t *out);

/* How many 8x8 tiles this context has rendered TWICE since it was created (synchronises the device).
 * The frame kernels evaluate fp64 divide / sqrt / normalise with shortened, correctly rounded sequences
 * that are valid for operands within about 1e+-70 of the scene's scale (chess2rt_amd/csrc/fp64_lean.h);
 * every use tests its operands, and a tile in which any lane met a zero numerator, an infinity, a NaN or
 * an operand beyond those windows discards its result and is rendered again with the compiler's IEEE
 * expansions — the same pixels as rounds 1-2 produced, at about twice the time for that tile.  A growing
 * number therefore costs speed, never correctness: e.g. a camera placed exactly on the plane of a cube face
 * (every ray's numerator for that face is 0).  Frames rendered with opts->count_rays take the IEEE path
 * only and do not count here. */
int c2rt_get_exact_redos(c2rt_ctx *ctx, uint64_t *out);

/* How many ground-only 8x8 tiles this context has handed from the short fp64 chain back to the full one since it
 * was created (synchronises the device).  Frames that look down on a floor from above, lit from above, compute a
 * floor hit through a short chain with a proven error bound (chess2rt_amd/csrc/ground_certain.h) and keep the
 * result only where every float and decision of the pixel is certain to be the full chain's; a tile with one
 * uncertain lane writes nothing and is rendered by the full chain at once.  A cost indicator like
 * c2rt_get_exact_redos, never a matter of correctness; about 1 tile in 3000 on the shipped scenes. */
int c2rt_get_ground_bails(c2rt_ctx *ctx, uint64_t *out);

/* How many sphere-interior 8x8 tiles this context has handed back to the general path since it was created
 * (synchronises the device).  A tile in which the mask pre-pass has proven that every primary ray's closest hit lies on
 * one sphere, and that nothing else can shadow it, is rendered by code that tests that sphere only
 * (chess2rt_amd/csrc/csg_void.h, "Sphere-interior tiles"); should a ray of such a tile miss the sphere after all, the
 * tile writes nothing and is rendered by the general path at once.  The proof says this stays 0; a cost indicator like
 * c2rt_get_exact_redos, never a matter of correctness. */
int c2rt_get_sphere_bails(c2rt_ctx *ctx, uint64_t *out);

/* How many 8x8 tiles that hold the ground and one leaf CsgOp node this context has handed back to the general path since
 * it was created (synchronises the device).  Such a tile is rendered by straight-line code for exactly those two nodes
 * (chess2rt_amd/csrc/c2rt_trace.inc: csg_tile); a tile in which a lane's CSG hit lists outgrow the wave's stack writes
 * nothing and is rendered by the general path at once.  0 on the shipped scenes; a cost indicator like
 * c2rt_get_exact_redos, never a matter of correctness. */
int c2rt_get_csg_tile_bails(c2rt_ctx *ctx, uint64_t *out);

/* Diagnostics: how many tiles that path has rendered since the context was created (synchronises the device).  Counted
 * by the lane-statistics build of the library only (chess2rt_amd/libc2rt_lanestats.so); 0 in every other build. */
int c2rt_get_csg_tiles(c2rt_ctx *ctx, uint64_t *out);

/* Pixel probe: mirrors `renderPixel` (rt/renderer.d:46-57): one sample at
 * integer (x, y), no AA, returns the colour and the trace result. */
int c2rt_render_pixel(c2rt_ctx *ctx, const c2rt_camera_frame *cam,
                      const c2rt_render_opts *opts, int x, int y,
                      c2rt_trace_result *out);

/* ---- ray queries: the caller's rays instead of a camera's ------------------ */

/* Most rays / segments one call takes; C2RT_ERR_LIMIT beyond. */
#define C2RT_MAX_RAYS (1u << 28)

typedef struct c2rt_ray     { double orig[3], dir[3]; } c2rt_ray;      /* 48 B */
typedef struct c2rt_segment { double from[3], to[3];  } c2rt_segment;  /* 48 B */
typedef struct c2rt_ray_hit {                                          /* 80 B */
    int32_t closest_node;          /* -1: no hit */
    int32_t leaf_geom;             /* IntersectionData.g (leaf geometry index), -1 without a hit */
    double dist, u, v;
    double p[3], normal[3];
} c2rt_ray_hit;

/* Ray i is `Renderer.trace(ray, TraceType.Ray)` (rt/renderer.d:325-376) with ray.orig = rays[i].orig, ray.dir =
 * rays[i].dir and depth 0, against the uploaded scene: data.dist starts at 1e99 (rt/renderer.d:333), the nodes are
 * tested in file order and the last one that returns true is the closest (rt/renderer.d:336-338).
 *   - `dir` is used EXACTLY AS GIVEN.  The reference's trace() does not normalise: Camera.getScreenRay has done so by
 *     then (rt/camera.d:144-147).  A caller who passes unit vectors built like getScreenRay's gets the frame's own
 *     rays — and the frame's own bits: the queries run the arithmetic the frames are held to.  For other lengths
 *     `dist` is whatever Node.intersect (rt/node.d:23-49) makes of them: it scales data.dist by the length of the
 *     direction in the node's space, normalises for Geometry.intersect and divides the hit distance by that length
 *     again, so `dist` counts lengths of `dir`; the shaders see `dir` as ray.dir (rt/shader.d:67-105,197-250).
 *   - hits[i] (nullable) is the TraceResult's record as c2rt_render_pixel reports it; without a hit closest_node and
 *     leaf_geom are -1, dist is 1e99 and the rest is 0.
 *   - rgb[i] (nullable; 3 floats per ray) is raytrace_impl's colour (rt/renderer.d:361-376): the closest node's
 *     shader's `shade`, with a shadow ray (Scene.testVisibility) towards every light, or the environment's black
 *     (rt/environment.d:7-10) without a hit.
 *   - a null `rgb` skips shading and its shadow rays altogether, a null `hits` the record stores; both null is
 *     C2RT_ERR_INVALID_ARG.
 * A ray made of NaNs, infinities or zeros terminates (every loop of the trace is bounded, C2RT_MAX_CSG_HITS) and
 * changes no other ray's result; its own record is whatever IEEE arithmetic makes of the reference's statements.
 *
 * Statuses, all decided before anything is enqueued or any caller pointer is read (the outputs are untouched):
 * n == 0 is C2RT_OK whatever the pointers; null `rays`, or both outputs null: C2RT_ERR_INVALID_ARG;
 * n > C2RT_MAX_RAYS: C2RT_ERR_LIMIT; no scene: C2RT_ERR_NO_SCENE.
 *
 * The _device variant takes device pointers and enqueues ONE kernel on `hip_stream` (a hipStream_t, NULL = default
 * stream): no host sync, no event left in the queue, ordered with the frames and queries on the same stream,
 * independent of those on other streams.  It needs no per-stream scratch (no tile masks, no retry list: the CSG
 * hit stacks have their full capacity) and keeps no reference to the stream.  On a multi-device context the queries
 * run on the lead device, as c2rt_render_pixel does. */
int c2rt_trace_rays_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n,
                           c2rt_ray_hit *hits_dev, float *rgb_dev, void *hip_stream);
/* The same from and into HOST memory: staged through the context's own stream in chunks of at most 2^18 rays (the
 * staging buffer holds one chunk of what is actually asked for, never n * 140 B); blocks until the results are there. */
int c2rt_trace_rays(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, c2rt_ray_hit *hits, float *rgb);

/* Segment i is `Scene.testVisibility(from, to)` (rt/scene.d:62-78): visible[i] = 1 when no node intersects the ray
 * from `from` towards `to` closer than |to - from|, else 0.  Statuses, streams and staging as above (`visible` is
 * required). */
int c2rt_test_visibility_device(c2rt_ctx *ctx, const c2rt_segment *seg_dev, uint64_t n,
                                uint8_t *visible_dev, void *hip_stream);
int c2rt_test_visibility(c2rt_ctx *ctx, const c2rt_segment *seg, uint64_t n, uint8_t *visible);

/* ---- hit planes: what every pixel of a camera frame hit -------------------- */

/* One plane per field of the TraceResult (rt/renderer.d:15-21) of the sample at integer (x, y) of every pixel:
 * what c2rt_render_pixel(x, y) reports, for the whole frame.  Row-major, local_rows x width, no padding.
 * Every pointer is nullable; at least one must be given.  A plane that is null is neither computed nor stored. */
typedef struct c2rt_hit_planes {
    int32_t *node;    /* [rows][W]     closest node, -1: no hit                         */
    int32_t *leaf;    /* [rows][W]     IntersectionData.g (leaf geometry), -1 without a hit */
    double  *dist;    /* [rows][W]     1e99 without a hit                               */
    double  *uv;      /* [rows][W][2]  0 without a hit                                  */
    double  *p;       /* [rows][W][3]                                                    */
    double  *normal;  /* [rows][W][3]  the geometric normal as the probe reports it (not face-forwarded) */
    float   *rgb;     /* [rows][W][3]  raytrace_impl's colour of that sample = the C2RT_TAPS_1 frame */
} c2rt_hit_planes;

/* Pixel (x, y) is the ray Camera.getScreenRay(x, y) (rt/camera.d:123-147: the pixel's integer corner, no 0.5), built
 * on the device from `cam` with the frame kernels' own arithmetic, sent through `trace` (rt/renderer.d:325-338) and,
 * for `rgb`, through raytrace_impl (rt/renderer.d:361-376): the values c2rt_render_pixel reports for a pinhole
 * camera, and the bits c2rt_trace_rays computes for that ray — without the 48 B per ray going in and without the
 * 80-byte records coming out for a caller who wants one field.
 *   - A pixel without a hit holds c2rt_ray_hit's record: node and leaf -1, dist 1e99, uv / p / normal 0; rgb is the
 *     environment's black (rt/environment.d:7-10).
 *   - opts: width, height, strip_height, strip_rank and strip_world mean what they mean for frames; with
 *     strip_world > 1 the planes hold this rank's rows only, compact, c2rt_local_rows(opts) of them.  `taps` must be a
 *     valid mode and is otherwise ignored (the sample at (x, y) is the first tap of every mode); `seed` is ignored.
 *   - rgb alone skips nothing of the trace but every record store; no rgb casts no shadow ray.
 *
 * Statuses, all decided before anything is enqueued or any plane is written, in this order: those of a frame call
 * (null camera or options, no scene: C2RT_ERR_NO_SCENE, bad size / tap mode / strip rank); null `planes`, or all seven
 * pointers null: C2RT_ERR_INVALID_ARG, each with its own message; C2RT_ERR_UNSUPPORTED with the cause named in
 * c2rt_last_error for cam->dof ("depth of field"), cam->stereo_separation != 0 ("stereo"), opts->count_rays
 * ("count_rays") and opts->prepass_bucket ("prepass_bucket"): a pixel's record is ONE ray's, and those modes have
 * many rays per pixel (or none of its own).
 *
 * The _device variant takes device pointers and enqueues ONE kernel on `hip_stream` (a hipStream_t, NULL = default
 * stream) under the rules of c2rt_trace_rays_device: no host sync, no event left in the queue, no per-stream scratch,
 * no reference kept to the stream; ordered with the frames and queries on the same stream.  On a multi-device context
 * it runs on the lead device, as c2rt_render_pixel and the queries do. */
int c2rt_render_hits_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                            const c2rt_hit_planes *planes_dev, void *hip_stream);
/* The same into HOST memory: staged through the context's staging buffer on the context's own stream in chunks of
 * whole rows of at most 2^18 pixels (the buffer holds one chunk of the planes actually asked for, at most 92 B per
 * pixel, whatever the frame size); blocks until the planes are there. */
int c2rt_render_hits(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                     const c2rt_hit_planes *planes_host);

/* Hit planes for a batch of cameras: c2rt_render_hits_device for n_frames frames in one launch, as
 * c2rt_render_frames_device is to c2rt_render_frame_device.  c2rt_hit_planes is unchanged; frame i's slice of a plane
 * starts i * local_rows * W * components elements behind the plane's pointer (components: 1 for node, leaf and dist,
 * 2 for uv, 3 for p, normal and rgb; local_rows = c2rt_local_rows(opts)).  Slices have no padding: with an odd width
 * the slice of frame i + 1 is aligned to nothing but its element.  Frame i's slice of every plane holds exactly the
 * bits c2rt_render_hits_device(ctx, &cams[i], opts, ...) writes; a plane whose pointer is null is neither computed nor
 * stored; nothing is written outside the n_frames slices.  Row strips (opts->strip_world > 1) work as in the
 * single-frame call: the slices hold this rank's rows, compact.
 *
 * Enqueued on `hip_stream`: one stream-ordered copy of the batch's table — n_frames parameter blocks — and ONE kernel
 * launch for all frames, the tiles of every frame in one grid, each reading its frame's block from the table.  The
 * table lives in the stream's scratch slot, as c2rt_render_frames_device's; no tile-mask table and no retry list are
 * used.  No host sync, no event left in the queue, no reference kept to the stream.  Blocking is
 * c2rt_render_frames_device's: the table goes to the device with a stream-ordered copy from pageable memory, so the call
 * may wait, on the host, until work enqueued EARLIER on `hip_stream` has drained (never for later work, never for other
 * streams); it also blocks when the slot's table has to grow (first call, more frames) or a 17th stream recycles a
 * slot.  Batches, single frames and hit batches on one stream stay ordered and may follow each other without a sync.
 *
 * Statuses, all decided before anything is enqueued or any plane is written, in this order: null context:
 * C2RT_ERR_INVALID_ARG; n_frames == 0: C2RT_OK whatever the other pointers are, nothing is read and nothing written;
 * those of c2rt_render_frames_device (null `cams` or `opts`; n_frames > C2RT_MAX_BATCH_FRAMES: C2RT_ERR_LIMIT; a
 * multi-device context, count_rays, prepass_bucket, a camera with depth of field or stereo: C2RT_ERR_UNSUPPORTED, the
 * last two naming the camera index and "depth of field" / "stereo"; a frame call's argument checks); null `planes`, or
 * all seven pointers null: C2RT_ERR_INVALID_ARG, each with its own message. */
int c2rt_render_frames_hits_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames,
                                   const c2rt_render_opts *opts, const c2rt_hit_planes *planes_dev, void *hip_stream);
/* The same into HOST memory, through the context's staging buffer on the context's own stream; the buffer never holds
 * more than one chunk of at most 2^18 pixels of the planes asked for (92 B per pixel, as c2rt_render_hits).  Where a
 * frame has at most 2^18 pixels a chunk is as many WHOLE frames as fit: one launch, one copy back per plane, one stream
 * sync per chunk.  Where a frame is larger, each frame goes in chunks of whole rows, as c2rt_render_hits.  Blocks until
 * the planes are there. */
int c2rt_render_frames_hits(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames,
                            const c2rt_render_opts *opts, const c2rt_hit_planes *planes_host);

/* Hit planes of a posed animation in one call: c2rt_render_frames_hits_device with a pose per frame, as
 * c2rt_render_frames_posed_device is to c2rt_render_frames_device.  Frame i's slices hold exactly the bits
 * c2rt_update_scene(&poses[i]) followed by c2rt_render_hits_device(&cams[i]) writes, each pose relative to the context's
 * scene as it is; the context's scene is unchanged by the call.  The table carries, behind the blocks and in the same
 * copy, the node and light tables of the frames whose poses change them.  Still ONE launch, whatever the poses: the
 * hit-plane kernel has no plane or identity instances, so c2rt_render_frames_posed_device's groups do not arise.
 * Statuses: those of c2rt_render_frames_hits_device in its order, then null `poses`: C2RT_ERR_INVALID_ARG, then those of
 * c2rt_update_scene for every poses[i], with "frame i: " in front of the message. */
int c2rt_render_frames_posed_hits_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses,
                                         uint32_t n_frames, const c2rt_render_opts *opts,
                                         const c2rt_hit_planes *planes_dev, void *hip_stream);
/* The same into HOST memory, as c2rt_render_frames_hits is to c2rt_render_frames_hits_device. */
int c2rt_render_frames_posed_hits(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses,
                                  uint32_t n_frames, const c2rt_render_opts *opts, const c2rt_hit_planes *planes_host);

/* ---- hit layers: every surface along a ray or pixel, in order --------------- */

/* Most layers one call walks; C2RT_ERR_LIMIT beyond. */
#define C2RT_MAX_HIT_LAYERS 16

/* All intersections along a ray, in order, in one launch: the reference's CsgOp.findAllIntersections
 * (rt/geometry.d:271-290) with the scene's `trace` (rt/renderer.d:325-338) in the place of geom.intersect.  For ray i:
 *
 *     o = ray.orig; d = ray.dir (never changed); total = 0.0
 *     for k in 0 .. max_layers-1:
 *         rec, colour = exactly what c2rt_trace_rays computes for the ray (o, d)
 *         if rec is a hit: rec.dist = rec.dist + total; total = rec.dist
 *         slot k := rec (a miss is c2rt_ray_hit's miss record: -1, -1, 1e99, zeros), colour slot k := colour (black for a miss)
 *         if rec is a miss: break
 *         o = rec.p + d * 1e-6          (componentwise, the product then the sum, not contracted)
 *     count = number of HIT records stored (0 .. max_layers)
 *
 *   - Layout, layer-major: layer k of ray i is hits[k * n + i], rgb[(k * n + i) * 3 ...]; count[i] is one byte per ray.
 *     hits + k * n is the array c2rt_trace_rays would fill for the rays of layer k.
 *   - Slot 0 of every output holds the bits of c2rt_trace_rays for that ray, hit or miss; with max_layers == 1 the call
 *     is c2rt_trace_rays plus `count`.
 *   - Slot k is written if and only if k <= count and k < max_layers: the miss that ended the walk is stored, nothing
 *     behind it is.  The _device variant does not touch the later slots; the host variant leaves them unspecified.
 *     READ `count`: it says how many slots of a ray mean something.
 *   - p, normal, u, v, closest_node and leaf_geom are the records of the stepped rays as they are.  Only `dist` is
 *     accumulated — rec.dist + total, one addition — WITHOUT the 1e-6 steps, as the reference does (temp.dist +=
 *     currentLength; currentLength = temp.dist): it counts lengths of `dir` from the first origin, short by the steps.
 *   - `dir` is used exactly as given, as for c2rt_trace_rays.
 *   - The walk is bounded by max_layers.  A ray of NaNs, zeros or 1e300, or one whose step does not move it (p + d *
 *     1e-6 == p finds the same surface again), ends there and changes no other ray's result.
 *   - Every output is nullable, not all three: a null `rgb` casts no shadow ray, a null `hits` stores no record, and
 *     `count` alone is a valid query ("how many surfaces").  What is written does not depend on which outputs are asked for.
 *   - No CSG hit list can overflow and there is no scratch: the same full-capacity hit stack as the other queries.
 *
 * Statuses, all decided before anything is enqueued or any caller pointer is read (the outputs are untouched), each
 * with its own message, in this order: those of c2rt_trace_rays (null context; n == 0 is C2RT_OK whatever else is
 * passed; null `rays`: C2RT_ERR_INVALID_ARG; n > C2RT_MAX_RAYS: C2RT_ERR_LIMIT; no scene: C2RT_ERR_NO_SCENE);
 * max_layers == 0: C2RT_ERR_INVALID_ARG; max_layers > C2RT_MAX_HIT_LAYERS: C2RT_ERR_LIMIT; all three outputs null:
 * C2RT_ERR_INVALID_ARG.
 *
 * The _device variant takes device pointers and enqueues ONE kernel on `hip_stream` under the rules of
 * c2rt_trace_rays_device: no host sync, no event, no scratch slot, nothing kept of the stream; on a multi-device
 * context, the lead device. */
int c2rt_trace_rays_layers_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n, uint32_t max_layers,
                                  c2rt_ray_hit *hits_dev, float *rgb_dev, uint8_t *count_dev, void *hip_stream);
/* The same from and into HOST memory: staged through the context's staging buffer in chunks of 2^18 / max_layers rays,
 * so the buffer never grows beyond what c2rt_trace_rays uses; each layer's slice of a chunk is copied to its place
 * (slots behind a ray's final miss hold unspecified bytes).  Blocks until the results are there. */
int c2rt_trace_rays_layers(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, uint32_t max_layers,
                           c2rt_ray_hit *hits, float *rgb, uint8_t *count);

/* The same for the pixels of a camera frame ("depth peeling"): plane k of a pixel is the k-th surface along the ray
 * c2rt_render_hits traces for it, by the definition above with c2rt_render_hits in the place of c2rt_trace_rays.
 * c2rt_hit_planes is unchanged; layer k's slice of a plane starts k * local_rows * W * components elements behind the
 * plane's pointer (the convention c2rt_render_frames_hits uses for frame i); count is [local_rows][W], one byte per
 * pixel.  Layer 0 of every plane holds the bits of c2rt_render_hits; all layers and `count` hold the bits of
 * c2rt_trace_rays_layers for the pixels' rays.  A pixel's slot k of a plane is written if and only if k <= count and
 * k < max_layers (read `count`).  Every plane and `count` are nullable, not all eight: a null plane is neither
 * computed nor stored, no rgb casts no shadow ray, `count` alone is valid.  Strips as in c2rt_render_hits.
 *
 * Statuses, in this order: those of a frame call; null `planes`: C2RT_ERR_INVALID_ARG; max_layers == 0:
 * C2RT_ERR_INVALID_ARG; max_layers > C2RT_MAX_HIT_LAYERS: C2RT_ERR_LIMIT; all seven planes and `count` null:
 * C2RT_ERR_INVALID_ARG; C2RT_ERR_UNSUPPORTED with the cause named for depth of field, stereo, count_rays and
 * prepass_bucket, worded as c2rt_render_hits words them.
 *
 * The _device variant: ONE kernel on `hip_stream`, no sync, no event, no scratch slot, nothing kept of the stream; on a
 * multi-device context, the lead device. */
int c2rt_render_hit_layers_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, uint32_t max_layers,
                                  const c2rt_hit_planes *planes_dev, uint8_t *count_dev, void *hip_stream);
/* The same into HOST memory: chunks of whole rows of at most 2^18 / max_layers pixels (at least one row) through the
 * context's staging buffer, each layer's slice of a chunk copied to its place; blocks until the planes are there. */
int c2rt_render_hit_layers(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, uint32_t max_layers,
                           const c2rt_hit_planes *planes_host, uint8_t *count_host);

/* ---- shading planes: the terms of a sample's colour, one plane each --------- */

/* One plane per term of Lambert.shade / Phong.shade (rt/shader.d:67-105, 197-250) of ONE sample.  Every pointer is
 * nullable; at least one must be given.  A plane that is null is neither computed nor stored. */
typedef struct c2rt_shade_planes {      /* 48 bytes */
    int32_t  *node;      /* [..]     closest node, -1: no hit (the hit planes' `node`)                                   */
    float    *albedo;    /* [..][3]  diffuseColor: texture.getTexColor(u, v) or shader.color        shader.d:74-76,202-203 */
    float    *light;     /* [..][3]  lightContrib when shade returns: ambient + every light's avgColor  shader.d:78-103,205-243 */
    float    *specular;  /* [..][3]  Phong's `specular` when shade returns (shader.d:207,244); +0,+0,+0 for a Lambert node */
    uint32_t *visible;   /* [..]     bit l (l < 32): light l passed `intensity() != 0 && testVisibility(p + N*1e-6, lightPos)` */
    float    *rgb;       /* [..][3]  shade's return value = the hit planes' `rgb` = the C2RT_TAPS_1 frame                  */
} c2rt_shade_planes;

/* What lies between the hit planes and the colour: the three locals of the reference's `shade` of the closest node at
 * its `return`, in fp32, computed by the statements the frames execute, and the lights that passed the shadow test.
 *   - Camera calls: the sample is the one c2rt_render_hits traces for pixel (x, y); planes are row-major
 *     [local_rows][W], strips as there.  Ray calls: the sample is ray i of c2rt_trace_rays, `dir` exactly as given;
 *     planes are [n].
 *   - rgb is albedo * light for a Lambert node and (albedo * light) + specular for a Phong node — the reference's own
 *     last statement — and has the bits of the hit planes' `rgb`, hence of the one-tap frame: on every hit the four
 *     colour planes satisfy that identity BIT FOR BIT in IEEE fp32 without contraction.
 *   - visible: bit l is set when light l < 32 passed the condition above.  A dark light's bit is clear and no shadow
 *     ray is cast for it, as in the reference; a visible light with cosTheta <= 0 has its bit set and adds zero.
 *     Lights 32 and beyond still add to `light` and `specular`; they have no bit.
 *   - A miss holds node -1, visible 0 and +0 in every float (rgb: the environment's black, rt/environment.d:7-10).
 *   - `node` and `albedo` alone cast no shadow ray and evaluate no light; the texture is read only when `albedo` or
 *     `rgb` is asked for.  What is written to one plane never depends on which others are asked for.
 *
 * Statuses, all decided before anything is enqueued or written.  Camera calls, in c2rt_render_hits' order and wording:
 * those of a frame call; null `planes`, or all six pointers null: C2RT_ERR_INVALID_ARG, each with its own message;
 * C2RT_ERR_UNSUPPORTED naming "depth of field", "stereo", "count_rays", "prepass_bucket".  Ray calls, in
 * c2rt_trace_rays' order: null context; n == 0 is C2RT_OK whatever else is passed; null `rays`: C2RT_ERR_INVALID_ARG;
 * n > C2RT_MAX_RAYS: C2RT_ERR_LIMIT; no scene: C2RT_ERR_NO_SCENE; then null `planes`, or all six pointers null:
 * C2RT_ERR_INVALID_ARG.
 *
 * The _device variants take device pointers and enqueue ONE kernel on `hip_stream`: no host sync, no event, no scratch
 * slot, nothing kept of the stream; on a multi-device context, the lead device.  The host variants go through the
 * context's staging buffer on the context's own stream in chunks of whole rows (or rays) of at most 2^18 samples —
 * at most 56 B per sample of planes — and block until the planes are there. */
int c2rt_render_shading_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                               const c2rt_shade_planes *planes_dev, void *hip_stream);
int c2rt_render_shading(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                        const c2rt_shade_planes *planes_host);
int c2rt_trace_rays_shading_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n,
                                   const c2rt_shade_planes *planes_dev, void *hip_stream);
int c2rt_trace_rays_shading(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, const c2rt_shade_planes *planes_host);

/* ---- occlusion planes: hemisphere visibility of every hit ------------------- */

/* Most visibility tests per sample; C2RT_ERR_LIMIT beyond (the mask is one 64-bit word). */
#define C2RT_MAX_OCCLUSION_SAMPLES 64

typedef struct c2rt_occlusion_opts {    /* 24 bytes */
    double   radius;     /* length of every sample's segment; finite and > 0 */
    uint64_t seed;       /* counter-RNG seed (opts->seed of a camera call is ignored, as the hit planes ignore it) */
    uint32_t samples;    /* K: 1 .. C2RT_MAX_OCCLUSION_SAMPLES */
    uint32_t reserved;   /* must be 0 */
} c2rt_occlusion_opts;

typedef struct c2rt_occlusion_planes {  /* 32 bytes; every pointer nullable, at least one given */
    int32_t  *node;      /* [..]     closest node, -1: no hit (the hit planes' `node`) */
    uint64_t *open;      /* [..]     bit s (s < K): sample s's segment is unoccluded; bits >= K are 0 */
    float    *ao;        /* [..]     (float)popcount(open) / (float)K */
    double   *bent;      /* [..][3]  sum, in sample order from +0, of the OPEN samples' directions; not normalised */
} c2rt_occlusion_planes;

/* Ambient occlusion of the closest hit of ONE sample: K segments of length `radius` from Lambert.spawnRay's origin
 * (p + N * 1e-6, rt/shader.d:118-135) along directions of hemisphereSample(N) (rt/shader.d:156-174), each answered by
 * Scene.testVisibility (rt/scene.d:62-78).  For sample index idx and ray (o, d) —
 *   camera calls: idx = FRAME row * W + column (strips and host chunks do not change it), (o, d) the ray
 *     c2rt_render_hits traces for the pixel; planes are row-major [local_rows][W], strips as there;
 *   ray calls: idx = the ray's index i in the caller's array (whatever chunk it travels in), `dir` exactly as given;
 *     planes are [n] —
 *
 *     rec = what c2rt_trace_rays computes for the ray (o, d)              -- node := rec.closest_node
 *     miss:  open = low K bits set, ao = 1.0f, bent = +0,+0,+0           -- nothing occludes the sky; no sample is drawn
 *     hit:   N    = dot(d, rec.normal) < 0 ? rec.normal : -rec.normal    -- faceforward, as shade() does
 *            from = rec.p + N * 1e-6
 *            key  = rng_key(occ.seed, idx, 0)
 *            for s in 0 .. K-1:
 *                u = rng_uniform(key, s, 0);  v = rng_uniform(key, s, 1)
 *                (sn, cs) = lens_sincos2pi(u)                             -- theta = 2 pi u
 *                w = 2.0 * v - 1.0;  c = sqrt(1.0 - w * w)                -- phi = acos(w) - pi/2: sin(phi) = -w, cos(phi) = c
 *                res = (cs * c, -w, sn * c)
 *                if ((res.x*N.x + res.y*N.y) + res.z*N.z) < 0: res = -res
 *                to = from + res * occ.radius                             -- product, then sum, not contracted
 *                if testVisibility(from, to): open |= 1 << s; bent += res -- c2rt_test_visibility's answer for (from, to)
 *            ao = (float)popcount(open) / (float)K
 *
 *   - Every operation is an IEEE fp64 +, * or sqrt without contraction, or one of the three routines of the lens samples
 *     (rng_key, rng_uniform, lens_sincos2pi: the counter RNG and the libm-free sine and cosine of 2 pi u); no libm call,
 *     so a CPU restatement produces the same bits.  Composition is the contract: the planes are what a caller gets who
 *     takes the records from c2rt_trace_rays, builds the segments as above and asks c2rt_test_visibility, BIT FOR BIT.
 *   - Build-defined, like the lens sample: the reference draws from rand() and goes through acos, cos and sin; the
 *     directions above are within 3.4e-15 per component of that formula evaluated by libm for the same (u, v), and of
 *     unit length within 1 ulp.
 *   - What is written to a plane never depends on which others are asked for; `node` alone traces no sample.
 *   - A lane of NaNs, zeros or 1e300 terminates (K bounded tests) and changes no other sample's result.
 *
 * Statuses, all decided before anything is enqueued or written, each with its own message.  Camera calls: those of a
 * frame call, in c2rt_render_hits' order; ray calls: those of c2rt_trace_rays, in its order (null context; n == 0 is
 * C2RT_OK whatever else is passed; null `rays`: C2RT_ERR_INVALID_ARG; n > C2RT_MAX_RAYS: C2RT_ERR_LIMIT; no scene:
 * C2RT_ERR_NO_SCENE).  Then, for both: null `occ`: C2RT_ERR_INVALID_ARG; radius NaN, infinite or <= 0:
 * C2RT_ERR_INVALID_ARG; samples == 0 or reserved != 0: C2RT_ERR_INVALID_ARG; samples > C2RT_MAX_OCCLUSION_SAMPLES:
 * C2RT_ERR_LIMIT; null `planes`, or all four pointers null: C2RT_ERR_INVALID_ARG.  Camera calls then:
 * C2RT_ERR_UNSUPPORTED naming "depth of field", "stereo", "count_rays", "prepass_bucket".
 *
 * The _device variants take device pointers and enqueue ONE kernel on `hip_stream`: no host sync, no event, no scratch
 * slot, nothing kept of the stream; on a multi-device context, the lead device; after c2rt_update_scene they see the
 * posed scene.  The host variants go through the context's staging buffer on the context's own stream in chunks of whole
 * rows (or rays) of at most 2^18 samples — at most 40 B per sample of planes — and block until the planes are there. */
int c2rt_render_occlusion_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                                 const c2rt_occlusion_opts *occ, const c2rt_occlusion_planes *planes_dev, void *hip_stream);
int c2rt_render_occlusion(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                          const c2rt_occlusion_opts *occ, const c2rt_occlusion_planes *planes_host);
int c2rt_trace_rays_occlusion_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n,
                                     const c2rt_occlusion_opts *occ, const c2rt_occlusion_planes *planes_dev, void *hip_stream);
int c2rt_trace_rays_occlusion(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n,
                              const c2rt_occlusion_opts *occ, const c2rt_occlusion_planes *planes_host);

/* ---- gather planes: one-bounce indirect diffuse light of every hit ----------- */

/* Most spawned rays per sample; C2RT_ERR_LIMIT beyond (the mask is one 64-bit word). */
#define C2RT_MAX_GATHER_SAMPLES 64

typedef struct c2rt_gather_opts {      /* 16 bytes */
    uint64_t seed;       /* counter-RNG seed (opts->seed of a camera call is ignored) */
    uint32_t samples;    /* K: 1 .. C2RT_MAX_GATHER_SAMPLES */
    uint32_t reserved;   /* must be 0 */
} c2rt_gather_opts;

typedef struct c2rt_gather_planes {    /* 32 bytes; every pointer nullable, at least one given */
    int32_t  *node;      /* [..]    closest node, -1: no hit (the hit planes' `node`) */
    uint64_t *hits;      /* [..]    bit s (s < K): sample s's ray hit a node; bits >= K are 0 */
    float    *indirect;  /* [..][3] mean weighted colour arriving over the hemisphere */
    float    *bounce;    /* [..][3] albedo * indirect: what to ADD to the frame's colour */
} c2rt_gather_planes;

/* One-bounce indirect diffuse light of the closest hit of ONE sample: K rays from Lambert.spawnRay's origin (p + N *
 * 1e-6, rt/shader.d:118-135) along directions of hemisphereSample(N) (rt/shader.d:156-174), each given the colour of
 * Renderer.raytrace — what c2rt_trace_rays returns as `rgb` — and the weight brdfEval / pdf of pathtrace_impl
 * (rt/renderer.d:451-460) without the albedo.  `frame + bounce` is a one-bounce global-illumination frame.  Sample index
 * idx and ray (o, d) are exactly the occlusion planes' —
 *   camera calls: idx = FRAME row * W + column (strips and host chunks do not change it), (o, d) the ray
 *     c2rt_render_hits traces for the pixel; planes are row-major [local_rows][W], strips as there;
 *   ray calls: idx = the ray's index i in the caller's array (whatever chunk it travels in), `dir` exactly as given;
 *     planes are [n] —
 *
 *     rec = what c2rt_trace_rays computes for (o, d)                      -- node := rec.closest_node
 *     miss, or the scene's max_trace_depth == 0:
 *            hits = 0, indirect = bounce = +0,+0,+0                       -- no sample is drawn
 *            (max_trace_depth == 0: the spawned ray has depth 1 and trace() returns black before
 *             intersecting anything, rt/renderer.d:330; node is still the record's)
 *     hit:   N    = dot(d, rec.normal) < 0 ? rec.normal : -rec.normal     -- faceforward
 *            from = rec.p + N * 1e-6
 *            key  = rng_key(seed, idx, 0)
 *            sum  = (+0f, +0f, +0f);  hits = 0
 *            for s in 0 .. K-1:
 *                res  = the occlusion planes' direction for (key, s, N)   -- same draws, same flip, same bits
 *                cosw = (res.x*N.x + res.y*N.y) + res.z*N.z               -- fp64
 *                w    = (float)(2.0 * cosw)                               -- brdfEval/pdf without the albedo:
 *                                                                            ((1/PI) * cos) / (1/(2 PI))
 *                (hit_s, L) = what c2rt_trace_rays reports for the ray (from, res), `dir` exactly as given:
 *                             closest_node >= 0, and its rgb
 *                if hit_s: hits |= 1 << s
 *                sum.c = sum.c + L.c * w        for c in r, g, b           -- fp32 multiply, then fp32 add, not contracted
 *            indirect.c = sum.c / (float)K
 *            bounce.c   = albedo.c * indirect.c                            -- albedo: the shading planes' `albedo` for (o, d)
 *
 *   - Composition is the contract: the planes are, BIT FOR BIT, what a caller gets who takes the records from
 *     c2rt_trace_rays, builds the K rays per hit as above, asks c2rt_trace_rays (records and rgb) for them, takes
 *     `albedo` from c2rt_trace_rays_shading and does the fp32 sums.  The definition uses no libm call of its own.
 *   - With the same seed the directions are those of the occlusion planes.  `res` is passed on un-normalised (it is of
 *     unit length within 1 ulp), because that is what the composed call sees.
 *   - The spawned rays are shaded with the full node mask and no ground shortcut, as every caller's ray is.
 *   - What is written to a plane never depends on which others are asked for.  `node` alone traces no sample; `node` +
 *     `hits` alone cast no shadow ray (the spawned rays' closest-hit search only); `indirect` without `bounce` fetches no
 *     primary albedo.
 *   - A lane of NaNs, zeros or 1e300 terminates (K bounded traces) and changes no other sample's result.
 *   - Build-defined, where the reference is not reproducible: the draws, as for the lens and occlusion samples; the
 *     rounding of `w` to fp32; that the path multiplier is applied at all (the reference's pathtrace(ray, multiplier)
 *     drops its second argument); that the spawned ray's colour is raytrace's — direct light by shadow rays — rather
 *     than a further bounce (with PointLight.solidAngle == 0, a black environment and lights that cannot be hit, every
 *     further bounce of the reference is black).  gi_enabled stays refused.
 *
 * Statuses, all decided before anything is enqueued or written, each with its own message.  Camera calls: those of a
 * frame call, in c2rt_render_hits' order; ray calls: those of c2rt_trace_rays, in its order (n == 0 is C2RT_OK whatever
 * else is passed).  Then, for both: null `g`, samples == 0 or reserved != 0: C2RT_ERR_INVALID_ARG; samples >
 * C2RT_MAX_GATHER_SAMPLES: C2RT_ERR_LIMIT; null `planes`, or all four pointers null: C2RT_ERR_INVALID_ARG.  Camera calls
 * then: C2RT_ERR_UNSUPPORTED naming "depth of field", "stereo", "count_rays", "prepass_bucket".
 *
 * The _device variants take device pointers and enqueue ONE kernel on `hip_stream`: no host sync, no event, no scratch
 * slot, nothing kept of the stream; on a multi-device context, the lead device; after c2rt_update_scene they see the
 * posed scene.  The host variants go through the context's staging buffer on the context's own stream in chunks of whole
 * rows (or rays) of at most 2^18 samples — at most 36 B per sample of planes — and block until the planes are there. */
int c2rt_render_gather_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                              const c2rt_gather_opts *g, const c2rt_gather_planes *planes_dev, void *hip_stream);
int c2rt_render_gather(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                       const c2rt_gather_opts *g, const c2rt_gather_planes *planes_host);
int c2rt_trace_rays_gather_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n,
                                  const c2rt_gather_opts *g, const c2rt_gather_planes *planes_dev, void *hip_stream);
int c2rt_trace_rays_gather(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n,
                           const c2rt_gather_opts *g, const c2rt_gather_planes *planes_host);

/* ---- path planes: multi-bounce indirect diffuse light of every hit ----------- */

/* Most paths per sample and most bounces per path; C2RT_ERR_LIMIT beyond. */
#define C2RT_MAX_PATHS        64
#define C2RT_MAX_PATH_BOUNCES  8

typedef struct c2rt_path_opts {        /* 16 bytes */
    uint64_t seed;       /* counter-RNG seed (opts->seed of a camera call is ignored) */
    uint32_t paths;      /* P: 1 .. C2RT_MAX_PATHS */
    uint32_t bounces;    /* B: 1 .. C2RT_MAX_PATH_BOUNCES; what is traced is Beff = min(B, scene max_trace_depth) */
} c2rt_path_opts;

typedef struct c2rt_path_planes {      /* 40 bytes; every pointer nullable, at least one given */
    int32_t  *node;      /* [..]    closest node, -1: no hit (the hit planes' `node`) */
    uint32_t *segments;  /* [..]    spawned segments that hit a node, over all paths and depths (<= P * Beff) */
    float    *indirect;  /* [..][3] mean weighted light arriving at the hit, all depths */
    float    *bounce;    /* [..][3] albedo * indirect */
    float    *radiance;  /* [..][3] rgb + bounce: the global-illumination frame itself */
} c2rt_path_planes;

/* Multi-bounce indirect diffuse light of the closest hit of ONE sample: renderSampleGI's pathsPerPixel paths of up to
 * maxTraceDepth bounces (rt/renderer.d:289-301, pathtrace_impl 378-463).  P paths leave the hit as the gather planes'
 * rays do; where a segment hits, the path goes on from Lambert.spawnRay's origin of that hit along another direction of
 * hemisphereSample, its throughput multiplied by the albedo of the vertex it leaves and by brdfEval / pdf without the
 * albedo.  Every segment is given the colour of Renderer.raytrace — what c2rt_trace_rays returns as `rgb`.  Sample index
 * idx and ray (o, d) are exactly the gather planes' —
 *   camera calls: idx = FRAME row * W + column (strips and host chunks do not change it), (o, d) the ray
 *     c2rt_render_hits traces for the pixel; planes are row-major [local_rows][W], strips as there;
 *   ray calls: idx = the ray's index i in the caller's array (whatever chunk it travels in), `dir` exactly as given;
 *     planes are [n] —
 *   and with Beff = min(bounces, the scene's max_trace_depth):
 *
 *     rec = what c2rt_trace_rays computes for (o, d)                      -- node := rec.closest_node
 *     miss, or Beff == 0:
 *            segments = 0, indirect = bounce = +0,+0,+0, radiance = the ray's c2rt_trace_rays rgb; nothing is drawn
 *     hit:   N0 = dot(d, rec.normal) < 0 ? rec.normal : -rec.normal       -- faceforward
 *            from0 = rec.p + N0 * 1e-6
 *            a0  = the shading planes' `albedo` for (o, d)
 *            sum = (+0f, +0f, +0f);  segments = 0
 *            for p in 0 .. P-1:                                           -- path-major ...
 *                from = from0;  N = N0
 *                for j in 0 .. Beff-1:                                    -- ... bounce-minor: this ORDER of the fp32
 *                                                                            sum is the contract
 *                    res  = the occlusion planes' direction for (rng_key(seed, idx, j), p, N)
 *                                                                         -- tap = depth, sample = path; j == 0: the
 *                                                                            gather planes' draws
 *                    w    = (float)(2.0 * ((res.x*N.x + res.y*N.y) + res.z*N.z))
 *                    T.c  = j == 0 ? w : (T.c * a.c) * w                  -- fp32, two multiplies in this order;
 *                                                                            a: albedo of the vertex just left
 *                    (r, L) = c2rt_trace_rays' record and rgb for the ray (from, res), `dir` exactly as given
 *                                                                         -- a miss: L = +0,+0,+0
 *                    sum.c = sum.c + L.c * T.c                            -- fp32 multiply, then fp32 add, not
 *                                                                            contracted; executed for a miss too
 *                    if r.closest_node < 0: break
 *                    segments += 1
 *                    a = the shading planes' `albedo` for (from, res)
 *                    N = dot(res, r.normal) < 0 ? r.normal : -r.normal;  from = r.p + N * 1e-6
 *            indirect.c = sum.c / (float)P
 *            bounce.c   = a0.c * indirect.c
 *            radiance.c = rgb.c + bounce.c                                -- rgb: c2rt_trace_rays' for (o, d)
 *
 *   - Composition is the contract: every plane is, BIT FOR BIT, what a caller gets from c2rt_trace_rays (records and
 *     rgb), c2rt_trace_rays_shading (`albedo`) and the fp32 arithmetic above.  No libm call of its own.
 *   - With bounces == 1 `indirect` and `bounce` are the gather planes' bits at samples == P and the same seed, and
 *     `segments` is the popcount of their `hits`.
 *   - Why Beff: the spawned ray at vertex j has depth j + 1, and trace() returns black before intersecting once the
 *     depth exceeds maxTraceDepth (rt/renderer.d:330).  max_trace_depth == 0 draws nothing.
 *   - What is written to a plane never depends on which others are asked for.  `node` alone traces no path; `node` +
 *     `segments` cast no shadow ray and fetch no albedo (closest-hit searches only); only `radiance` casts the primary
 *     hit's shadow rays.
 *   - A lane of NaNs, zeros or 1e300 ends after at most P * Beff segments and changes no other sample's result.
 *   - Build-defined: the gather planes' list (the draws, the rounding of `w`, that the multiplier is applied at all,
 *     that every vertex takes raytrace's direct light from all lights — the reference's one random light has
 *     solidAngle == 0 and contributes nothing), and two more: every material continues the path as Lambert does (the
 *     reference's Phong.spawnRay is assert(0)); the primary ray is not jittered (renderSampleGI's x + uniform * dx is
 *     what the sample tables are for).  gi_enabled stays refused.
 *
 * Statuses, all decided before anything is enqueued or written, each with its own message.  Camera calls: those of a
 * frame call, in c2rt_render_hits' order; ray calls: those of c2rt_trace_rays, in its order (n == 0 is C2RT_OK whatever
 * else is passed).  Then, for both: null `g`, paths == 0, bounces == 0: C2RT_ERR_INVALID_ARG; paths > C2RT_MAX_PATHS,
 * bounces > C2RT_MAX_PATH_BOUNCES: C2RT_ERR_LIMIT, in this order; null `planes`, or all five pointers null:
 * C2RT_ERR_INVALID_ARG.  Camera calls then: C2RT_ERR_UNSUPPORTED naming "depth of field", "stereo", "count_rays",
 * "prepass_bucket".
 *
 * The _device variants take device pointers and enqueue ONE kernel on `hip_stream`: no host sync, no event, no scratch
 * slot, nothing kept of the stream; on a multi-device context, the lead device; after c2rt_update_scene they see the
 * posed scene.  The host variants go through the context's staging buffer on the context's own stream in chunks of whole
 * rows (or rays) of at most 2^18 samples — at most 44 B per sample of planes — and block until the planes are there. */
int c2rt_render_paths_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                             const c2rt_path_opts *g, const c2rt_path_planes *planes_dev, void *hip_stream);
int c2rt_render_paths(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                      const c2rt_path_opts *g, const c2rt_path_planes *planes_host);
int c2rt_trace_rays_paths_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n,
                                 const c2rt_path_opts *g, const c2rt_path_planes *planes_dev, void *hip_stream);
int c2rt_trace_rays_paths(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n,
                          const c2rt_path_opts *g, const c2rt_path_planes *planes_host);

/* ---- counted path planes: a number of paths per sample ----------------------- */

/* The path planes with ONE BYTE per sample beside them that says how many paths the sample gets: `counts`, required —
 *   camera calls: row-major [local_rows][W], strips as for the planes;  ray calls: [n].
 * Everything else — sample index, ray, seed, bounces, planes — is the path call's.  With c = min(counts[i], g->paths)
 * (g->paths is the cap and keeps its range 1 .. C2RT_MAX_PATHS):
 *
 *   c >= 1:  every plane of sample i is, BIT FOR BIT, what c2rt_render_paths / c2rt_trace_rays_paths writes for that
 *            sample with paths = c, the same seed, bounces and sample index: path p of sample idx draws
 *            rng_key(seed, idx, j) with sample p whatever P is, the fp32 sum is path-major, and indirect = sum / (float)c.
 *   c == 0:  the sample takes the path contract's "miss, or Beff == 0" line: `node` is still the record's,
 *            segments = 0, indirect = bounce = +0,+0,+0, radiance = the ray's c2rt_trace_rays rgb; nothing is drawn.
 *
 *   - A counts plane whose every value is >= g->paths gives the uniform call's bits.
 *   - The path planes' rules hold: what is written to a plane does not depend on which others are asked for; `node` alone
 *     traces no path (and reads no count); a lane of NaNs ends after at most c * Beff segments.
 *
 * Launch order.  A wavefront runs as long as its heaviest lane, so one sample at 64 paths among 63 at 2 costs its wave 64
 * paths' worth of iterations.  The _device variants take `scratch_dev`, nullable:
 *   null:      natural order — the path call's lane mapping, ONE kernel, nothing else enqueued;
 *   non-null:  count order — c2rt_paths_counted_scratch_bytes(samples of the call: local_rows * W, or n) bytes, 16-byte
 *              aligned, written by the call.  A counting sort of the sample indices by c, heaviest class first, is
 *              enqueued ahead of the path kernel (one memset, three small kernels), and lane i of the path kernel takes
 *              the i-th sample of that order; a camera call derives the pixel from the index.  The order inside a class
 *              is left to atomics.  A call of 2^32 samples or more runs in natural order all the same.
 * Both orders write the same bits: no sample's value depends on where it ran.  Which one is faster depends on how the
 * counts lie in the plane (profiles/paths_counted.md).
 *
 * c2rt_paths_counted_scratch_bytes: pure host arithmetic, no context: 512 + 4 * n_samples rounded up to 16.
 *
 * Statuses, all decided before anything is enqueued or written: the path call's own first, in its order (n == 0 of a
 * ray call is C2RT_OK whatever else is passed); then null `counts`: C2RT_ERR_INVALID_ARG; then, for the _device variants,
 * a non-null `scratch_dev` that is not 16-byte aligned: C2RT_ERR_INVALID_ARG.
 *
 * The stream rules are the path calls'.  The host variants stage the counts of each chunk beside the chunk's planes —
 * one more byte per sample — with the scratch behind them (4 B per sample and 544 B per chunk) and run every chunk in count
 * order: on the three uneven planes measured it took 0.43 to 0.76 of natural order's time, on an even plane 1.07
 * (profiles/paths_counted.md). */
size_t c2rt_paths_counted_scratch_bytes(uint64_t n_samples);
int c2rt_render_paths_counted_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                                     const c2rt_path_opts *g, const uint8_t *counts_dev, const c2rt_path_planes *planes_dev,
                                     void *scratch_dev, void *hip_stream);
int c2rt_render_paths_counted(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                              const c2rt_path_opts *g, const uint8_t *counts, const c2rt_path_planes *planes_host);
int c2rt_trace_rays_paths_counted_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n,
                                         const c2rt_path_opts *g, const uint8_t *counts_dev, const c2rt_path_planes *planes_dev,
                                         void *scratch_dev, void *hip_stream);
int c2rt_trace_rays_paths_counted(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n,
                                  const c2rt_path_opts *g, const uint8_t *counts, const c2rt_path_planes *planes_host);

/* ---- denoise: edge-aware a-trous filter of a Monte-Carlo plane, guided by the hit planes ---- */

/* Most levels of one call; C2RT_ERR_LIMIT beyond (level l taps 2^l pixels apart). */
#define C2RT_MAX_DENOISE_LEVELS 8

typedef struct c2rt_denoise_guides {   /* 40 bytes */
    const int32_t *node;     /* [H][W]     required: the hit planes' `node`, < 0: no hit */
    const double  *normal;   /* [H][W][3]  required: the hit planes' `normal`, exactly as c2rt_render_hits writes it */
    const double  *p;        /* [H][W][3]  required: the hit planes' `p` */
    const float   *albedo;   /* [H][W][channels]  nullable: multiplied into the result (the shading planes' `albedo`) */
    const float   *base;     /* [H][W][channels]  nullable: added to the result (the hit planes' `rgb`) */
} c2rt_denoise_guides;

typedef struct c2rt_denoise_opts {     /* 32 bytes */
    uint32_t width, height;        /* the WHOLE frame: no strips (a caller who renders in strips de-interleaves first) */
    uint32_t levels;               /* 0 .. C2RT_MAX_DENOISE_LEVELS; 0: the two closing steps alone */
    uint32_t channels;             /* 1 | 3 (1: the occlusion planes' `ao`) */
    uint32_t normal_power_log2;    /* 0 .. 7: the normal term is dot(n, n')^(2^this) */
    float    sigma_plane;          /* finite, > 0: distance from the centre's tangent plane at which a tap weighs half */
    float    sigma_colour;         /* finite, >= 0; 0: no colour term */
    uint32_t reserved;             /* 0 */
} c2rt_denoise_opts;

/* An edge-avoiding a-trous wavelet filter: a 5x5 B3-spline with dilation 2^l per level, its edge-stopping terms computed
 * in fp32 from the hit planes, which are on the device anyway.  All planes are full-frame, row-major [H][W], and `in` and
 * `out` are float[channels] per pixel.  The arithmetic is the contract — fp32, no libm call, no exp, no contraction, IEEE
 * divide, subnormals kept — and tests/denoise_reference.py restates it in numpy to the bit:
 *
 *   per pixel, once:  nf.c = (float)normal.c,  pf.c = (float)p.c
 *   per call:         K = {1/16, 1/4, 3/8, 1/4, 1/16};  inv_plane = 1f / sigma_plane
 *   per level l:      sc = sigma_colour * 2^-l;  inv_c2 = 1f / (sc * sc)
 *
 *   level l, step s = 1 << l, plane C to plane D, pixel q = (x, y):
 *     node[q] < 0:  D[q] = C[q] (the bits)
 *     else: sumw = +0f; sum.c = +0f
 *       for j in -2..2: for i in -2..2:            -- this ORDER of the fp32 sums is the contract
 *         t = (x + i*s, y + j*s); outside the frame: skip
 *         (i, j) == (0, 0): w = K[2]*K[2]          -- the centre always counts, none of the tests below
 *         else:
 *           node[t] != node[q]: skip
 *           dn = (nf[q].x*nf[t].x + nf[q].y*nf[t].y) + nf[q].z*nf[t].z;   !(dn > 0): skip
 *           wn = dn; normal_power_log2 times: wn = wn * wn
 *           d.c = pf[t].c - pf[q].c;  dp = (nf[q].x*d.x + nf[q].y*d.y) + nf[q].z*d.z
 *           e = dp * inv_plane;  wp = 1f / (1f + e*e)
 *           w = ((K[i+2]*K[j+2]) * wn) * wp        -- K[i+2]*K[j+2] is exact in fp32
 *           sigma_colour > 0:  dc.c = C[t].c - C[q].c;  d2 = (dc.r*dc.r + dc.g*dc.g) + dc.b*dc.b   (one channel: dc*dc)
 *                              w = w * (1f / (1f + d2 * inv_c2))
 *           !(w > 0): skip                          -- NaN, and underflow to zero
 *         sum.c = sum.c + w * C[t].c;  sumw = sumw + w     -- multiply, then add; not contracted
 *       D[q].c = sum.c / sumw
 *
 *   Levels 0 .. levels-1 run in order, from `in` to `out` through `out` itself and one more plane in the scratch; `in`
 *   and the guides are never written.  Then, for EVERY pixel (misses included), fused into the last store:
 *     albedo given:  v.c = albedo.c * v.c
 *     base given:    v.c = base.c + v.c
 *   levels == 0 does these two steps alone: with the path planes' `indirect` as `in`, the shading planes' `albedo` and the
 *   hit planes' `rgb` as `base`, `out` is the path planes' `radiance` bit for bit.
 *
 *   - A NaN or infinite colour reaches exactly the pixels this arithmetic says; a NaN normal or a `p` beyond fp32 drops
 *     the taps it makes NaN and never the centre.
 *   - The step may exceed the frame: then only the centre is inside, and D[q].c = (w*C[q].c) / w.
 *
 * c2rt_denoise_scratch_bytes: pure host arithmetic, no context.  0 for options c2rt_denoise_device would refuse, and
 * for levels == 0 (then `scratch_dev` may be null).  Otherwise width * height * (32 + (levels > 1 ? 4 * channels : 0)):
 * the guides packed to fp32 once — per pixel (nf, the bits of node) and (pf, 0), two 16-byte words — and, behind them, the
 * one ping-pong plane that levels > 1 need beside `out`.  At most 44 B per pixel.  `scratch_dev` must be 16-byte aligned.
 *
 * c2rt_denoise_device needs no uploaded scene.  It takes the stream rules of c2rt_render_hits_device (no host sync, no
 * event, nothing kept of the stream, the lead device of a multi-device context), enqueues levels + 1 kernels for
 * levels >= 1 and one for levels == 0, and writes only `out_dev` and `scratch_dev`.
 *
 * Statuses, all decided before anything is enqueued or written, each with its own message, in this order.
 * C2RT_ERR_INVALID_ARG: null context; null `opts`; null `guides`; width or height 0; channels not 1 or 3; sigma_plane
 * NaN, infinite or <= 0; sigma_colour NaN, infinite or < 0; reserved != 0.  C2RT_ERR_LIMIT: levels >
 * C2RT_MAX_DENOISE_LEVELS; normal_power_log2 > 7.  C2RT_ERR_INVALID_ARG again: null `node`, `normal` or `p`; null `in`;
 * null `out`; out == in; out == scratch; in == scratch (both for a non-null scratch); null scratch where
 * c2rt_denoise_scratch_bytes is not 0; a scratch that is not 16-byte aligned. */
size_t c2rt_denoise_scratch_bytes(const c2rt_denoise_opts *o);
int c2rt_denoise_device(c2rt_ctx *ctx, const c2rt_denoise_guides *guides_dev, const c2rt_denoise_opts *o,
                        const float *in_dev, float *out_dev, void *scratch_dev, void *hip_stream);
/* The same from and into HOST memory, the scratch the library's own: guides, `in`, `out` and the scratch go through the
 * context's grow-only staging buffer on the context's own stream, whole (at most 144 B per pixel; nothing is allocated
 * once the buffer is large enough); blocks until `out` is there.  The same statuses without the scratch's. */
int c2rt_denoise(c2rt_ctx *ctx, const c2rt_denoise_guides *guides_host, const c2rt_denoise_opts *o, const float *in, float *out);

/* The global-illumination frame in one call, denoised: on the device, the hit planes (node, normal, p, rgb), the shading
 * planes' `albedo`, the path planes' `indirect` and the filter with albedo and base = rgb; 12 B per pixel come back.
 * out_rgb[H][W][3] is bit for bit what a caller composes from c2rt_render_hits, c2rt_render_shading, c2rt_render_paths
 * and c2rt_denoise.  Statuses, in this order: those of c2rt_render_paths without the planes' (a frame call's, the path
 * options'); null `d`, null `out_rgb`: C2RT_ERR_INVALID_ARG; C2RT_ERR_UNSUPPORTED naming "depth of field", "stereo",
 * "count_rays", "prepass_bucket", then "strip_world" for opts->strip_world > 1 (0 and 1 both mean the whole frame, as everywhere); d->width / d->height other than the
 * frame's, d->channels != 3: C2RT_ERR_INVALID_ARG; then c2rt_denoise's for `d`.  Staged whole through the context's
 * staging buffer (144 B per pixel); blocks until the frame is there. */
int c2rt_render_paths_denoised(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                               const c2rt_path_opts *g, const c2rt_denoise_opts *d, float *out_rgb);

/* ---- temporal accumulation: reproject the previous frame's history, fold the new sample into a running mean ---- */

/* Largest max_age; C2RT_ERR_LIMIT beyond (an age is exact in fp32 far beyond it; the bound keeps 1 / N away from 2^-24). */
#define C2RT_MAX_TEMPORAL_AGE 65535

typedef struct c2rt_temporal_opts {    /* 32 bytes */
    uint32_t width, height;        /* the WHOLE frame: no strips */
    uint32_t channels;             /* 1 | 3 */
    uint32_t max_age;              /* 1 .. C2RT_MAX_TEMPORAL_AGE: the running mean's N stops growing here (1: no accumulation) */
    float    min_normal_dot;       /* finite, 0 <= . < 1: a history tap counts only if dot(n, n') > this */
    float    max_plane_dist;       /* finite, > 0: ... and only if it lies this close to the pixel's tangent plane */
    uint32_t reserved[2];          /* 0 */
} c2rt_temporal_opts;

typedef struct c2rt_temporal_guides {  /* 24 bytes: the CURRENT frame's hit planes, all required */
    const int32_t *node;     /* [H][W]     the hit planes' `node`, < 0: no hit */
    const double  *normal;   /* [H][W][3]  the hit planes' `normal`, exactly as c2rt_render_hits writes it */
    const double  *p;        /* [H][W][3]  the hit planes' `p` */
} c2rt_temporal_guides;

typedef struct c2rt_temporal_planes {  /* 24 bytes: the outputs, each nullable */
    float    *colour;        /* [H][W][channels]  the accumulated plane */
    float    *variance;      /* [H][W]  temporal variance of the luminance */
    uint32_t *age;           /* [H][W]  samples behind the pixel: 0 miss, 1 no history, .. max_age */
} c2rt_temporal_planes;

/* Every pixel's world point `p` is projected into the PREVIOUS camera; the previous call's accumulated value is fetched
 * there, bilinearly, from the taps that lie on the same surface; the new sample `in` is folded into a running mean whose
 * count stops at max_age.  The stage traces nothing and needs no uploaded scene.  All planes are full-frame, row-major
 * [H][W]; `in` and `colour` are float[channels] per pixel.
 *
 * The history is the state between two calls.  The caller owns two of them and swaps them; the layout is part of the
 * contract, planar over px = width * height pixels, c2rt_temporal_history_bytes = px * (32 + 4 * channels + 8) bytes,
 * 16-byte aligned:
 *   g0[px]            float4  (nf.x, nf.y, nf.z, the bits of the int32 node)
 *   g1[px]            float4  (pf.x, pf.y, pf.z, the bits of the uint32 age)
 *   c[px][channels]   float   the accumulated colour (what `colour` holds)
 *   m[px]             float2  (M1, M2): the running means of the luminance and of its square
 * nf and pf are the filter's "per pixel, once" conversions: nf.c = (float)normal.c, pf.c = (float)p.c.
 *
 * The arithmetic is the contract — the reprojection in fp64, the gather in fp32, no libm call, no contraction, IEEE
 * divides, subnormals kept — and tests/temporal_reference.py restates it in numpy to the bit:
 *
 *   per call, on the host, in fp64 (they invert Camera.getScreenRay, rt/camera.d:140-145: with p - pos = a A + b U + c V the
 *   screen position is (W b / a, H c / a), and det cancels out of the quotients):
 *     A = prev.up_left - prev.pos;  U = prev.up_right - prev.up_left;  V = prev.down_left - prev.up_left
 *     na = cross(U, V);  nb = cross(V, A);  nc = cross(A, U)        -- cross(a, b).x = a.y*b.z - a.z*b.y, and so on
 *     det = (A.x*na.x + A.y*na.y) + A.z*na.z;  Wd = (double)width;  Hd = (double)height
 *
 *   pixel q = (x, y):
 *     node[q] < 0 (a miss):  colour = in[q] (the bits); M1 = M2 = variance = +0f; age = 0
 *     else:
 *       r.c = p[q].c - prev.pos.c
 *       ka = (r.x*na.x + r.y*na.y) + r.z*na.z;  kb, kc likewise with nb, nc
 *       s = det > 0 ? ka : -ka;                                    !(s > 0): NO HISTORY  (behind the camera, at its eye, NaN)
 *       sx = (kb / ka) * Wd;  sy = (kc / ka) * Hd
 *       !(sx > -1.0 && sx < Wd && sy > -1.0 && sy < Hd):           NO HISTORY
 *       x0 = floor(sx); fx = (float)(sx - x0);  y0 = floor(sy); fy = (float)(sy - y0)
 *       wx = {1f - fx, fx};  wy = {1f - fy, fy}
 *       sumw = sum.c = s1 = s2 = +0f;  amin = UINT32_MAX
 *       for j in 0..1: for i in 0..1:               -- this ORDER of the fp32 sums is the contract
 *         t = (x0 + i, y0 + j); outside the frame: skip
 *         w = wx[i] * wy[j];                                       !(w > 0): skip   -- zero, NaN, underflow
 *         the history's node[t] != node[q]: skip
 *         dn = (nf[q].x*hn.x + nf[q].y*hn.y) + nf[q].z*hn.z;       !(dn > min_normal_dot): skip     -- hn = the history's nf[t]
 *         d.c = hp.c - pf[q].c;  dp = (nf[q].x*d.x + nf[q].y*d.y) + nf[q].z*d.z                     -- hp = the history's pf[t]
 *         !(fabsf(dp) <= max_plane_dist): skip
 *         sumw = sumw + w;  sum.c = sum.c + w * hc.c;  s1 = s1 + w * hM1;  s2 = s2 + w * hM2        -- multiply, then add
 *         amin = min(amin, the history's age[t])
 *       !(sumw > 0):                                               NO HISTORY
 *       h.c = sum.c / sumw;  m1 = s1 / sumw;  m2 = s2 / sumw
 *       n = min(amin + 1, max_age)  (without wrapping);  a = 1f / (float)n
 *       colour.c = h.c + (in.c - h.c) * a
 *       lum = (0.2126f*in.r + 0.7152f*in.g) + 0.0722f*in.b          (one channel: lum = in)
 *       M1 = m1 + (lum - m1) * a;  M2 = m2 + (lum*lum - m2) * a
 *       v = M2 - M1*M1;  variance = v > 0 ? v : +0f;  age = n
 *     NO HISTORY:  colour = in[q] (the bits);  M1 = lum;  M2 = lum*lum;  variance = +0f;  age = 1
 *   the history out takes (nf, node), (pf, age), colour and (M1, M2) of EVERY pixel, misses included.
 *   history_prev == NULL (the first frame) makes every hit pixel NO HISTORY; prev_cam may then be null as well.
 *
 *   - max_age == 1 passes `in` through (a = 1: colour = h + (in - h), within an ulp of in); a large max_age is the plain
 *     running mean of everything seen on the surface.
 *   - A NaN normal or a `p` beyond fp32 drops the taps it makes NaN; a NaN `in` reaches its own pixel now and, through
 *     the history, the pixels that fetch it later.
 *   - What is NOT promised: a node moved by c2rt_update_scene between two frames keeps its index and, in THIS call,
 *     simply fails the plane test where it moved far enough — it restarts, nothing follows it.  Following it is
 *     c2rt_temporal_accumulate_motion's part, and posed sequences are c2rt_render_paths_sequence_posed*'s (below).  Out
 *     of scope everywhere: any clamp of the history against the new frame's neighbourhood.
 *
 * c2rt_temporal_history_bytes: pure host arithmetic, no context; 0 for options c2rt_temporal_accumulate_device refuses.
 *
 * c2rt_temporal_accumulate_device takes the stream rules of c2rt_denoise_device (no host sync, no event, nothing kept of
 * the stream, the lead device of a multi-device context, no uploaded scene), enqueues ONE kernel and writes only
 * `history_out_dev` and the planes given.  `prev_cam` and `o` are host memory, read before the call returns.
 *
 * Statuses, all decided before anything is enqueued or written, each with its own message, in this order.
 * C2RT_ERR_INVALID_ARG: null context; null `o`; null `guides`; width or height 0; channels not 1 or 3; min_normal_dot NaN,
 * infinite, < 0 or >= 1; max_plane_dist NaN, infinite or <= 0; reserved != 0.  C2RT_ERR_LIMIT: max_age 0 or above
 * C2RT_MAX_TEMPORAL_AGE.  C2RT_ERR_INVALID_ARG again: null `node`, `normal` or `p`; null `in`; null `history_out`; null
 * `planes` (a struct of three null pointers is fine: the history alone); a non-null `history_prev` with a null
 * `prev_cam`; with a history, det zero or not finite ("degenerate previous camera"); history_out == history_prev;
 * colour == in; a history (either) that is not 16-byte aligned. */
size_t c2rt_temporal_history_bytes(const c2rt_temporal_opts *o);
int c2rt_temporal_accumulate_device(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_dev,
                                    const c2rt_temporal_opts *o, const float *in_dev, const void *history_prev_dev,
                                    void *history_out_dev, const c2rt_temporal_planes *planes_dev, void *hip_stream);
/* The same from and into HOST memory, the histories as host byte blobs of c2rt_temporal_history_bytes: guides, `in`, both
 * histories and the planes go through the context's grow-only staging buffer on the context's own stream, whole (at most
 * 188 B per pixel; nothing is allocated once the buffer is large enough); blocks until the planes and `history_out` are
 * there.  The same statuses; a host history needs no alignment. */
int c2rt_temporal_accumulate(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_host,
                             const c2rt_temporal_opts *o, const float *in, const void *history_prev, void *history_out,
                             const c2rt_temporal_planes *planes_host);

/* ---- temporal accumulation that follows moved nodes ---- */

/* Most moved nodes of one call; C2RT_ERR_LIMIT beyond. */
#define C2RT_MAX_MOTION_NODES 16

typedef struct c2rt_temporal_motion {  /* 32 bytes; host memory, read before the call returns */
    uint32_t n_nodes;                  /* 0 .. C2RT_MAX_MOTION_NODES moved nodes */
    uint32_t reserved;                 /* 0 */
    const uint32_t *node_index;        /* [n_nodes], distinct; the values the `node` plane holds */
    const double   *prev_transform;    /* [n_nodes][30], c2rt_scene_desc::node_transform layout: the pose the HISTORY was made under */
    const double   *cur_transform;     /* [n_nodes][30]: the pose the current guides were rendered under */
} c2rt_temporal_motion;

/* c2rt_temporal_accumulate* for a scene whose nodes moved between the two frames (c2rt_update_scene, a posed sequence):
 * a pixel that lies on a listed node is carried back through the node's motion — out of the current pose into the node's
 * own space, from there into the previous pose — before it is projected into the previous camera, so that it finds the
 * history the same piece of surface left, wherever the node was then.  History layout, c2rt_temporal_history_bytes, the
 * planes and every pixel whose node is not listed are c2rt_temporal_accumulate's, to the bit; a history written by
 * either call is read by the other.  `motion` NULL or n_nodes == 0: the call IS c2rt_temporal_accumulate* (the same
 * kernel).  The stage still needs no uploaded scene, allocates nothing and enqueues ONE kernel; the motion records
 * travel with the launch, as its arguments.
 *
 * The arithmetic is the contract, in the terms of c2rt_temporal_accumulate's (no libm call, no contraction, IEEE divides,
 * subnormals kept); tests/temporal_motion_reference.py restates it in numpy to the bit.  Matrices are row-major 3x3,
 * M[i][j] = m[3*i + j], and multiply a ROW vector from the right as the reference's mul(v, M) does (Transform.point,
 * undoPoint, normal: rt/transform.d:57-81).  The library never inverts a matrix: it uses the caller's four parts.
 *
 *   per moved node m, on the host, in fp64, from cur = cur_transform[m] and prev = prev_transform[m]:
 *     Tc = cur.transform;  Ic = cur.inverseTransform;  oc = cur.offset
 *     Tp = prev.transform;  TIp = prev.transposedInverse;  op = prev.offset
 *     R[i][j] = (Ic[i][0]*Tp[0][j] + Ic[i][1]*Tp[1][j]) + Ic[i][2]*Tp[2][j]       -- R = Ic . Tp: undoPoint of cur, then point of prev
 *     N[i][j] = (Tc[0][i]*TIp[0][j] + Tc[1][i]*TIp[1][j]) + Tc[2][i]*TIp[2][j]     -- N = transpose(Tc) . TIp: the normal likewise
 *
 *   pixel q whose node[q] is not listed:  c2rt_temporal_accumulate's arithmetic and bits.
 *   pixel q with node[q] == node_index[m], in fp64:
 *     e.c  = p[q].c - oc.c
 *     p'.j = ((e.x*R[0][j] + e.y*R[1][j]) + e.z*R[2][j]) + op.j
 *     n'.j = (normal[q].x*N[0][j] + normal[q].y*N[1][j]) + normal[q].z*N[2][j]
 *     r.c = p'.c - prev.pos.c, and the chain of c2rt_temporal_accumulate from there on: ka, kb, kc, s, sx, sy, x0, y0, fx, fy
 *     pf'.c = (float)p'.c;  nf'.c = (float)n'.c;  l2 = (nf'.x*nf'.x + nf'.y*nf'.y) + nf'.z*nf'.z           -- fp32 from here on
 *     mn2 = min_normal_dot * min_normal_dot;  mp2 = max_plane_dist * max_plane_dist
 *     a tap, behind the frame, weight and node tests (the history's node[t] != node[q]: skip, as there):
 *       dn = (nf'.x*hn.x + nf'.y*hn.y) + nf'.z*hn.z;                !(dn > 0 && dn*dn > mn2 * l2): skip
 *       d.c = hp.c - pf'.c;  dp = (nf'.x*d.x + nf'.y*d.y) + nf'.z*d.z;   !(dp*dp <= mp2 * l2): skip
 *     the sums, the running mean, the moments and the planes as there.
 *   the history out takes the CURRENT (nf, node), (pf, age) of every pixel, as there: n' and p' are never stored.
 *
 *   - n' is a unit vector only under a rigid motion, hence the squared tests with n's own length in them and no square
 *     root; under a rigid motion they are the static call's tests up to rounding.
 *   - A NaN or an infinity in a listed transform is not refused: it makes the chain of that node's pixels NaN, and they
 *     take NO HISTORY (age 1); a zero matrix sends every pixel of the node to one point with l2 = 0, and the normal test
 *     drops every tap.  No other pixel is touched by either.
 *   - The history lags what it was made of: a light moved between the frames, or the shadow a moved node casts on a
 *     node that did not move, changes `in` while the old mean is still fetched — the running mean follows at its own
 *     pace.  A clamp of the history against the new frame is out of scope.
 *
 * Statuses: c2rt_temporal_accumulate_device's, in its order, and behind its "null `planes`": motion->reserved != 0:
 * C2RT_ERR_INVALID_ARG; n_nodes > C2RT_MAX_MOTION_NODES: C2RT_ERR_LIMIT; n_nodes > 0 with a null node_index,
 * prev_transform or cur_transform: C2RT_ERR_INVALID_ARG; an index listed twice: C2RT_ERR_INVALID_ARG (c2rt_last_error
 * names the entry).  A motion without a history is fine and ignored.  The device variant keeps the stream rules of
 * c2rt_temporal_accumulate_device, the host variant the staging of c2rt_temporal_accumulate. */
int c2rt_temporal_accumulate_motion_device(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_dev,
                                           const c2rt_temporal_opts *o, const c2rt_temporal_motion *motion, const float *in_dev,
                                           const void *history_prev_dev, void *history_out_dev, const c2rt_temporal_planes *planes_dev,
                                           void *hip_stream);
int c2rt_temporal_accumulate_motion(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_host,
                                    const c2rt_temporal_opts *o, const c2rt_temporal_motion *motion, const float *in,
                                    const void *history_prev, void *history_out, const c2rt_temporal_planes *planes_host);

/* A global-illumination SEQUENCE in one call: for each i, on the device, the hit planes of cams[i] (node, normal, p, rgb),
 * the shading planes' `albedo`, the path planes' `indirect` with seed g->seed + i, the accumulation of `indirect` (prev_cam
 * = &cams[i - 1] and frame i - 1's history; frame 0 has neither), and the filter of the accumulated plane with albedo and
 * base = rgb into out_rgb[i]; 12 B per pixel and frame come back.  out_rgb[n_frames][H][W][3] is bit for bit what a caller
 * composes from c2rt_render_hits, c2rt_render_shading, c2rt_render_paths, c2rt_temporal_accumulate and c2rt_denoise.  The
 * two histories live in the context's staging buffer beside the frame's planes (248 B per pixel in all, whatever
 * n_frames); blocks until the last frame is there.  Statuses, in this order: those of c2rt_render_paths_denoised for
 * cams[0] (null `cams` is its null camera); n_frames == 0: C2RT_ERR_INVALID_ARG; null `t`; t->width / t->height other
 * than the frame's, t->channels != 3: C2RT_ERR_INVALID_ARG; then the temporal options' own; then, for every later camera,
 * C2RT_ERR_UNSUPPORTED naming "depth of field" or "stereo", and "degenerate previous camera" for every camera but the last. */
int c2rt_render_paths_sequence(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                               const c2rt_path_opts *g, const c2rt_temporal_opts *t, const c2rt_denoise_opts *d, float *out_rgb);

/* ---- variance-guided denoise: the a-trous filter steered by the temporal stage's variance and age planes ---- */

/* Largest min_age; C2RT_ERR_LIMIT beyond (the boost min_age / age of a young pixel's spatial estimate stays a small number). */
#define C2RT_MAX_VARIANCE_MIN_AGE 64

typedef struct c2rt_denoise_variance_opts {   /* 40 bytes */
    uint32_t width, height;        /* the WHOLE frame: no strips */
    uint32_t levels;               /* 0 .. C2RT_MAX_DENOISE_LEVELS; 0: the variance estimate and the two closing steps alone */
    uint32_t channels;             /* 1 | 3 */
    uint32_t normal_power_log2;    /* 0 .. 7, as c2rt_denoise_opts */
    float    sigma_plane;          /* finite, > 0, as c2rt_denoise_opts */
    float    sigma_lum;            /* finite, >= 0: luminance differences are measured in local standard deviations times this; 0: no luminance term */
    float    var_floor;            /* finite, > 0: added to the scaled variance, so that a pixel without variance still divides */
    uint32_t min_age;              /* 0 .. C2RT_MAX_VARIANCE_MIN_AGE: pixels younger than this get the spatial estimate; 0: none */
    uint32_t reserved;             /* 0 */
} c2rt_denoise_variance_opts;

/* c2rt_denoise with the colour term replaced by a LUMINANCE term whose scale is the pixel's own standard deviation: the
 * caller no longer tunes sigma_colour to a noise level that differs from pixel to pixel, the temporal stage's `variance`
 * plane says what it is.  The variance is filtered alongside the colour (it is what the next level's term reads), and a
 * pixel too young for a temporal variance (age < min_age) gets a spatial one from its 7x7 neighbourhood.  The guides are
 * c2rt_denoise_guides, unchanged.  Beside them:
 *   variance      [H][W]            float   required   the temporal planes' `variance`
 *   age           [H][W]            uint32  nullable   the temporal planes' `age`; null, or min_age == 0: no spatial estimate
 *   in            [H][W][channels]  float   required
 *   out           [H][W][channels]  float   required
 *   variance_out  [H][W]            float   nullable   the variance after the last level
 *
 * The arithmetic is the contract, in c2rt_denoise's idiom — fp32, no libm call, no exp, no sqrt, no contraction, IEEE
 * divide, subnormals kept, the order of every sum fixed — and tests/denoise_variance_reference.py restates it in numpy to
 * the bit.  nf, pf, K, inv_plane, dn, wn, wp and the node test are exactly c2rt_denoise's (above).
 *
 *   lum(x) = (0.2126f*x.r + 0.7152f*x.g) + 0.0722f*x.b        (one channel: lum(x) = x; the temporal stage's coefficients)
 *   per call:  sl2 = sigma_lum * sigma_lum
 *
 *   Stage A, the variance estimate V0, pixel q = (x, y):
 *     node[q] < 0:                                          V0[q] = +0f
 *     age == NULL, or min_age == 0, or age[q] >= min_age:   V0[q] = variance[q] (the bits)
 *     else (the spatial estimate, over 7x7 ADJACENT pixels of `in`):
 *       sumw = s1 = s2 = +0f
 *       for j in -3..3: for i in -3..3:                     -- this ORDER of the fp32 sums is the contract
 *         t = (x + i, y + j); outside the frame: skip
 *         (i, j) == (0, 0): w = 1f                          -- the centre always counts
 *         else: node[t] != node[q]: skip;  dn as the filter's, !(dn > 0): skip;  wn, wp as the filter's
 *               w = wn * wp;  !(w > 0): skip
 *         l = lum(in[t]);  s1 = s1 + w*l;  s2 = s2 + w*(l*l);  sumw = sumw + w
 *       m1 = s1 / sumw;  m2 = s2 / sumw;  v = m2 - m1*m1;  v = v > 0 ? v : +0f        -- a NaN becomes +0f
 *       V0[q] = v * ((float)min_age / (float)max(age[q], 1u))
 *
 *   Stage B, level l, step s = 1 << l, planes (C, V) to (D, V'), pixel q:
 *     node[q] < 0:  D[q] = C[q], V'[q] = V[q] (the bits)
 *     else:
 *       sigma_lum > 0:
 *         G = {1/16, 1/8, 1/16;  1/8, 1/4, 1/8;  1/16, 1/8, 1/16};  gs = gw = +0f
 *         for j in -1..1: for i in -1..1:  t = (x + i, y + j)       -- ADJACENT pixels whatever the step; no node test
 *           inside the frame:  gs = gs + G[j][i]*V[t];  gw = gw + G[j][i]
 *         g = gs / gw;  inv_l = 1f / (sl2 * g + var_floor);  lq = lum(C[q])
 *       sumw = sv = +0f;  sum.c = +0f
 *       the 25 taps in c2rt_denoise's order, with its skips and its w = ((K[i+2]*K[j+2]) * wn) * wp (no colour term); then
 *         sigma_lum > 0 (not for the centre):  dl = lum(C[t]) - lq;  w = w * (1f / (1f + (dl*dl) * inv_l))
 *         !(w > 0): skip
 *         sum.c = sum.c + w*C[t].c;  sumw = sumw + w;  sv = sv + (w*w)*V[t]
 *       (the centre always counts, w = K[2]*K[2], in all three sums)
 *       D[q].c = sum.c / sumw;  V'[q] = sv / (sumw * sumw)
 *
 *   Levels 0 .. levels-1 run in order from (`in`, V0).  c2rt_denoise's two closing steps (albedo, base) are fused into the
 *   last colour store, for every pixel; they do not touch the variance.  `variance_out` is V after the last level; with
 *   levels == 0 it is V0, and `out` is the two closing steps alone.
 *
 *   - A NaN, negative or infinite `variance` reaches exactly the taps this arithmetic says: through g the pixels whose 3x3
 *     holds it, through sv the pixels that keep it as a tap.
 *   - A zero or NaN sl2*g + var_floor drops every tap but the centre (inv_l is infinite or NaN, every tap's w zero or NaN).
 *     A NEGATIVE one — only a negative `variance` makes it — gives x = (dl*dl) * inv_l < 0: a tap with x > -1 keeps a
 *     factor above 1, x == -1 exactly makes it 1f / +0f = +inf (kept, and sumw infinite), x < -1 makes it negative and the
 *     tap is dropped.  The arithmetic is followed to the bit either way; a caller who wants sense clamps the variance.
 *   - variance_out is the variance a sum of INDEPENDENT samples would have.  After level 0 the taps are correlated, and it
 *     underestimates what is left (on a flat plane of unit-variance noise, 4 levels: 1e-6 against a measured 2.5e-5).  It is
 *     a relative guide for the next level's term, not an error bar.
 *
 * c2rt_denoise_variance_scratch_bytes: pure host arithmetic, no context; 0 for options c2rt_denoise_variance_device would
 * refuse.  Otherwise width * height * ((levels > 0 || min_age > 0 ? 32 : 0) + (levels > 1 ? 4 * channels : 0) +
 * (levels > 0 ? 8 : 0) + (levels > 1 ? 4 : 0)): c2rt_denoise's packed guides (the levels read them, and so does the spatial
 * estimate), its colour ping-pong plane, and behind them the variance planes: V0 and g, the 3x3-blurred variance of the
 * level about to run, and for levels > 1 a second V to alternate with.  At most 56 B per pixel.  `scratch_dev` must be
 * 16-byte aligned.
 *
 * c2rt_denoise_variance_device takes c2rt_denoise_device's stream rules (no host sync, no event, nothing kept of the
 * stream, no uploaded scene, the lead device of a multi-device context) and writes only `out_dev`, `variance_out_dev` and
 * `scratch_dev`.  It enqueues levels + 2 kernels for levels >= 1 (the packing, stage A, one per level) and with
 * sigma_lum > 0 one more per level (the 3x3 blur of V ahead of it): 2 levels + 2.  For levels == 0 it enqueues the closing
 * steps' one and ahead of it, only where variance_out is given, stage A and (with `age` and min_age > 0) the packing: 1 to 3.
 *
 * Statuses, all decided before anything is enqueued or written, each with its own message, in this order.
 * C2RT_ERR_INVALID_ARG: null context; null `o`; null `guides`; width or height 0; channels not 1 or 3; sigma_plane NaN,
 * infinite or <= 0; sigma_lum NaN, infinite or < 0; var_floor NaN, infinite or <= 0; reserved != 0.  C2RT_ERR_LIMIT:
 * levels > C2RT_MAX_DENOISE_LEVELS; normal_power_log2 > 7; min_age > C2RT_MAX_VARIANCE_MIN_AGE.  C2RT_ERR_INVALID_ARG
 * again: null `node`, `normal` or `p`; null `variance`; null `in`; null `out`; out == in; variance_out == variance;
 * out == scratch; variance_out == scratch (both for a non-null scratch); null scratch where
 * c2rt_denoise_variance_scratch_bytes is not 0; a scratch that is not 16-byte aligned; in == scratch; variance == scratch
 * (both for a non-null scratch: the packing launch would overwrite the input). */
size_t c2rt_denoise_variance_scratch_bytes(const c2rt_denoise_variance_opts *o);
int c2rt_denoise_variance_device(c2rt_ctx *ctx, const c2rt_denoise_guides *guides_dev, const c2rt_denoise_variance_opts *o,
                                 const float *variance_dev, const uint32_t *age_dev, const float *in_dev, float *out_dev,
                                 float *variance_out_dev, void *scratch_dev, void *hip_stream);
/* The same from and into HOST memory, the scratch the library's own: guides, `variance`, `age`, `in`, both outputs and the
 * scratch go through the context's grow-only staging buffer on the context's own stream, whole (at most 168 B per pixel;
 * nothing is allocated once the buffer is large enough); blocks until `out` and `variance_out` are there.  The same
 * statuses without the scratch's. */
int c2rt_denoise_variance(c2rt_ctx *ctx, const c2rt_denoise_guides *guides_host, const c2rt_denoise_variance_opts *o,
                          const float *variance, const uint32_t *age, const float *in, float *out, float *variance_out);

/* c2rt_render_paths_sequence with the loop closed: the temporal stage also writes its `variance` and `age` planes, and the
 * filter is c2rt_denoise_variance, fed by them (no variance_out).  out_rgb[n_frames][H][W][3] is bit for bit what a caller
 * composes from c2rt_render_hits, c2rt_render_shading, c2rt_render_paths, c2rt_temporal_accumulate and
 * c2rt_denoise_variance.  The two histories live in the staging buffer beside the frame's planes (268 B per pixel in all,
 * whatever n_frames; allocated once, before the first launch); blocks until the last frame is there.  Statuses:
 * c2rt_render_paths_sequence's, in its order, with `dv` in place of `d` ("null denoise options", dv->width / dv->height
 * other than the frame's, dv->channels != 3, then c2rt_denoise_variance's own for the options).  Strips and multi-device
 * sharding are refused as there. */
int c2rt_render_paths_sequence_variance(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                                        const c2rt_path_opts *g, const c2rt_temporal_opts *t, const c2rt_denoise_variance_opts *dv,
                                        float *out_rgb);

/* The two sequence calls for a POSED animation: frame i is the context's current scene with poses[i] applied — each pose
 * relative to the current scene, as in c2rt_render_frames_posed — seen through cams[i]; the context's scene is unchanged
 * when the call returns.  Per frame, on the context's stream: the pose update (c2rt_update_scene's own path: the base
 * scene patched by poses[i], planned on the host, the changed tables copied in stream order, nothing allocated), the hit
 * planes, albedo and `indirect` with seed g->seed + i, c2rt_temporal_accumulate_motion against frame i - 1's camera and
 * history, and the filter; after the last frame the base pose is put back the same way.  Frame i's motion list (i >= 1):
 * every node poses[i - 1] or poses[i] names, in ascending order of its index, prev = its transform under poses[i - 1] (the
 * base's where poses[i - 1] does not name it), cur likewise under poses[i]; an entry whose 60 doubles are bytewise equal
 * is dropped.  Lights may be posed: the history then lags the lighting (above).  out_rgb[i] is bit for bit what a caller
 * composes from c2rt_update_scene (the base patched by poses[i]), c2rt_render_hits, c2rt_render_shading,
 * c2rt_render_paths, c2rt_temporal_accumulate_motion and c2rt_denoise (c2rt_denoise_variance for the second call).
 * Statuses, all decided before anything is enqueued or changed: those of the unposed call, in its order; null `poses`:
 * C2RT_ERR_INVALID_ARG; those of c2rt_update_scene for every poses[i], with "frame i: " in front of the message; more than
 * C2RT_MAX_MOTION_NODES entries in a frame's motion list: C2RT_ERR_LIMIT, naming the frame.  Strips and multi-device
 * sharding are refused as there. */
int c2rt_render_paths_sequence_posed(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, uint32_t n_frames,
                                     const c2rt_render_opts *opts, const c2rt_path_opts *g, const c2rt_temporal_opts *t,
                                     const c2rt_denoise_opts *d, float *out_rgb);
int c2rt_render_paths_sequence_posed_variance(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses,
                                              uint32_t n_frames, const c2rt_render_opts *opts, const c2rt_path_opts *g,
                                              const c2rt_temporal_opts *t, const c2rt_denoise_variance_opts *dv, float *out_rgb);

/* ---- adaptive path counts: the temporal variance steers the sampler ---------- */

typedef struct c2rt_path_count_opts {   /* 32 bytes */
    uint32_t min_paths;           /* 1 .. C2RT_MAX_PATHS */
    uint32_t max_paths;           /* min_paths .. C2RT_MAX_PATHS */
    uint32_t young_paths;         /* 1 .. C2RT_MAX_PATHS: no history, or younger than min_age */
    uint32_t min_age;             /* 0 .. C2RT_MAX_TEMPORAL_AGE */
    float    paths_per_variance;  /* finite, > 0 */
    uint32_t prev_paths;          /* 1 .. C2RT_MAX_PATHS: the count behind every history pixel where prev_counts is null */
    uint32_t reserved[2];         /* 0 */
} c2rt_path_count_opts;

/* How many paths each pixel of a frame should get, decided BEFORE the frame's paths are traced, from what the PREVIOUS
 * history says about the variance at the point the pixel sees now: the counts plane of c2rt_render_paths_counted.  It is
 * the first half of c2rt_temporal_accumulate's pixel — the reprojection and the four-tap gather of (M1, M2, age) — without
 * the fold; nothing is accumulated and no history is written.  The stage traces nothing and needs no uploaded scene.
 * `guides` are the CURRENT frame's hit planes; of `o`, width, height, channels (the history's layout), min_normal_dot and
 * max_plane_dist are used and max_age is ignored; `history_prev` (nullable: the first frame) is the history the previous
 * c2rt_temporal_accumulate call wrote, `prev_cam` its camera; `prev_counts` (nullable, uint8 [H][W]) the counts the
 * history's LAST sample was traced with.  Outputs: `counts` uint8 [H][W], required; `variance` float [H][W] and `age`
 * uint32 [H][W], each nullable.
 *
 * The arithmetic is the contract, as the temporal stage's is, and tests/path_counts_reference.py restates it in numpy to
 * the bit:
 *
 *   node[q] < 0:                    counts = 0; variance = +0f; age = 0
 *   else: the temporal contract's pixel, word for word, from `r.c = p[q].c - prev.pos.c` to `!(sumw > 0): NO HISTORY`,
 *         gathering s1, s2, amin (sum.c is not needed), and beside them
 *           cprev = max over the KEPT taps of (prev_counts ? prev_counts[t] : prev_paths);  cprev == 0: cprev = 1
 *     NO HISTORY (also: history_prev == NULL), or amin < min_age:
 *                                   counts = young_paths; variance = +0f; age = NO HISTORY ? 0 : amin
 *     else: m1 = s1 / sumw; m2 = s2 / sumw; v = m2 - m1*m1; v = v <= 0 ? +0f : v       -- a NaN stays a NaN (the
 *                                                                              accumulation's own variance clamps it to +0)
 *           t = (v * (float)cprev) * paths_per_variance                    -- fp32, two multiplies in this order
 *           !(t < (float)max_paths):  k = max_paths                        -- NaN and infinity land here: a history
 *                                                                              with a NaN moment asks for the most
 *           else: k = (uint32)t (truncation);  if ((float)k < t) k += 1;  k = max(k, min_paths)
 *           counts = k; variance = v; age = amin
 *
 *   - `age` is the history's own (the accumulation of the same frame reports min(age + 1, max_age)); `variance` is the
 *     gathered one, before this frame's sample is folded in.
 *   - Why cprev is in the rule: the history's variance is that of the per-frame SAMPLE, a mean over that frame's paths.
 *     Without the factor the rule is c' = K / c, which oscillates; with it the fixed point is
 *     c = paths_per_variance * (the variance of one path).  The running moments mix frames traced with different counts,
 *     so the estimate is exact only once the counts have settled.
 *   - Why min_paths >= 1: a pixel traced with 0 paths would fold a zero into the temporal mean.
 *   - Moved nodes (c2rt_temporal_accumulate_motion's list) are not followed: a pixel on a moved node fails the plane test
 *     here and gets young_paths, which is the safe side.
 *
 * Statuses, all decided before anything is enqueued or written, each with its own message, in this order:
 * c2rt_temporal_accumulate's for the context, `o`, `guides`, the sizes, channels, min_normal_dot, max_plane_dist and
 * reserved (max_age is not looked at); null `pc`: C2RT_ERR_INVALID_ARG; min_paths 0, max_paths < min_paths, young_paths 0:
 * C2RT_ERR_INVALID_ARG, and min_paths, max_paths or young_paths above C2RT_MAX_PATHS: C2RT_ERR_LIMIT, field by field in
 * the struct's order; min_age above C2RT_MAX_TEMPORAL_AGE: C2RT_ERR_LIMIT; prev_paths 0: C2RT_ERR_INVALID_ARG, above
 * C2RT_MAX_PATHS: C2RT_ERR_LIMIT; paths_per_variance NaN, infinite or <= 0, then reserved != 0: C2RT_ERR_INVALID_ARG; null
 * `node`, `normal` or `p`; null `counts`; a non-null `history_prev` with a null `prev_cam`; with a history, a degenerate
 * previous camera; on the device variant a history that is not 16-byte aligned: C2RT_ERR_INVALID_ARG.
 *
 * c2rt_path_counts_device takes c2rt_temporal_accumulate_device's stream rules and enqueues ONE kernel.  The host variant
 * stages everything whole through the context's staging buffer (at most 110 B per pixel) and blocks until the planes are
 * there; a host history needs no alignment. */
int c2rt_path_counts_device(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_dev,
                            const c2rt_temporal_opts *o, const c2rt_path_count_opts *pc, const void *history_prev_dev,
                            const uint8_t *prev_counts_dev, uint8_t *counts_dev, float *variance_dev, uint32_t *age_dev,
                            void *hip_stream);
int c2rt_path_counts(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_host,
                     const c2rt_temporal_opts *o, const c2rt_path_count_opts *pc, const void *history_prev,
                     const uint8_t *prev_counts, uint8_t *counts, float *variance, uint32_t *age);

/* c2rt_render_paths_sequence_variance with the sampler in the loop.  Frame 0 is traced with pc->young_paths everywhere,
 * through the counted call.  Frame i > 0: the hit planes; c2rt_path_counts from history i - 1, cams[i - 1] and the counts
 * of frame i - 1; c2rt_render_paths_counted with g->paths as the cap and seed g->seed + i; the accumulation; the variance
 * filter.  out_rgb is bit for bit the composition of the single calls.  The two count planes and the count-order scratch
 * sit in the staging buffer beside the rest: 6 B per pixel more, 274 in all; frame 0, whose counts are even, runs in natural
 * order and every later frame in count order.  Statuses:
 * c2rt_render_paths_sequence_variance's, in its order; then null `pc`; then the count options' own, in c2rt_path_counts'
 * order; then pc->max_paths > g->paths: C2RT_ERR_INVALID_ARG.  Posed sequences are not part of this call. */
int c2rt_render_paths_sequence_adaptive(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                                        const c2rt_path_opts *g, const c2rt_temporal_opts *t, const c2rt_denoise_variance_opts *dv,
                                        const c2rt_path_count_opts *pc, float *out_rgb);

/* ---- adaptive anti-aliasing: refine only the pixels the edge test flags ----- */

/* tooDifferent's default threshold — rt/color.d:18 */
#define C2RT_AA_THRESHOLD_REF 0.1f

/* Renderer.renderRT's three passes (rt/renderer.d:132-188) with the third run where the second raised its flag.  The
 * reference computes needsAA[x, y] and then refines every pixel; the flag is dead there, so no reference output pins
 * it, and what is specified here is the reference's statements read as written.  For a pinhole, mono camera, the
 * whole frame and opts->taps == C2RT_TAPS_REF5:
 *   1. out[y][x] is the C2RT_TAPS_1 frame: the bits c2rt_render_frame_device writes for `cam` with taps = 1.
 *   2. Detection (rt/renderer.d:154-177, tooDifferent rt/color.d:18-23).  neighs = { out[x, y], out[x > 0 ? x - 1 : x, y],
 *      out[x + 1 < W ? x + 1 : x, y], out[x, y > 0 ? y - 1 : y], out[x, y + 1 < H ? y + 1 : y] }; per channel, in fp32,
 *      average = ((((0 + n0) + n1) + n2) + n3) + n4, then / 5.0f; needs_aa[y][x] = 1 when for some i and channel
 *      fabsf(neighs[i].c - average.c) > threshold (the difference rounded to fp32; a NaN difference does not flag),
 *      else 0.  All five neighbours are values of step 1.
 *   3. Refinement (renderPixelAA, rt/renderer.d:233-251) of the flagged pixels only: accum = out[y][x]; accum +=
 *      sample(x + dx[s], y + dy[s]) for s = 1..4 in that order; out[y][x] = accum / 5.0f.
 * So a flagged pixel holds the bits of the C2RT_TAPS_REF5 frame and an unflagged pixel the bits of the C2RT_TAPS_1
 * frame.  needs_aa is W * H bytes, row-major, every byte written 0 or 1.
 *
 * Statuses, all decided before anything is enqueued or written, in this order: those of a frame call (null camera or
 * options, no scene: C2RT_ERR_NO_SCENE, bad size / tap mode / strip rank); C2RT_ERR_INVALID_ARG for taps !=
 * C2RT_TAPS_REF5, a threshold that is negative or NaN, a null output (needs_aa_dev included); C2RT_ERR_UNSUPPORTED with
 * the cause named in c2rt_last_error for cam->dof ("depth of field"), cam->stereo_separation != 0 ("stereo"),
 * opts->count_rays ("count_rays"), opts->prepass_bucket ("prepass_bucket"), opts->strip_world > 1 ("strip_world": the
 * neighbour rows belong to other ranks) and a context of c2rt_init_multi ("multi-device").
 *
 * The _device variant takes device pointers and enqueues, in order, on `hip_stream` (a hipStream_t, NULL = default
 * stream): the one-tap frame exactly as c2rt_render_frame_device does (tile-mask pre-pass, nested-CSG retry and the
 * stream's scratch slot included), the detection kernel and the refinement kernel.  No host sync, no event left in the
 * queue, no reference kept to the stream, and no scratch beyond the frame call's: the caller's needs_aa_dev is the
 * buffer between detection and refinement, which is why it is required here. */
int c2rt_render_frame_adaptive_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                                      float threshold, float *out_rgb_dev, uint8_t *needs_aa_dev, void *hip_stream);
/* The same into HOST memory: frame and flags are staged in the context's staging buffer on the context's own stream and
 * copied back once each (`needs_aa` is nullable here); blocks until they are there.  `stop_flag` is polled once, before
 * the launches; C2RT_ERR_CANCELLED leaves the outputs untouched. */
int c2rt_render_frame_adaptive(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                               float threshold, float *out_rgb, uint8_t *needs_aa, const volatile uint8_t *stop_flag);

/* Adaptive anti-aliasing for a batch: c2rt_render_frames_device and c2rt_render_frame_adaptive_device in one call.  Frame i
 * occupies out_rgb_dev + i * W * H * 3 floats and its flags needs_aa_dev + i * W * H bytes; both hold exactly the bits
 * c2rt_render_frame_adaptive_device(ctx, &cams[i], opts, threshold, ...) writes: every mask byte 0 or 1, the neighbours
 * of the edge test clamped at the frame's own edges, nothing written beyond frame n_frames - 1.
 *
 * Enqueued on `hip_stream`, in order: the one-tap batch exactly as c2rt_render_frames_device enqueues it with taps =
 * C2RT_TAPS_1 (table copy, mask pre-pass, frame launch or launches), ONE detection launch for all frames, ONE
 * refinement launch for all frames — the flagged tiles of every frame in one grid, reading their parameter blocks from
 * the batch's table, which carries one more block per frame in the same copy.  No host sync, no event left in the
 * queue, no reference kept to the stream.  Blocking, streams and scratch are c2rt_render_frames_device's: the table
 * goes to the device with a stream-ordered copy from pageable memory, so the call may wait, on the host, until work
 * enqueued EARLIER on `hip_stream` has drained (never for later work, never for other streams); it also blocks when the
 * stream's scratch has to grow (first call, more frames, a larger frame) or a 17th stream recycles a slot.  Batches
 * and single frames on one stream stay ordered and may follow each other without a sync.
 *
 * Statuses, all decided before anything is enqueued or written, in this order: those of c2rt_render_frames_device
 * (n_frames == 0 is C2RT_OK and writes nothing; n_frames > C2RT_MAX_BATCH_FRAMES: C2RT_ERR_LIMIT; depth of field,
 * stereo, count_rays, prepass_bucket and a multi-device context: C2RT_ERR_UNSUPPORTED); C2RT_ERR_INVALID_ARG for taps
 * != C2RT_TAPS_REF5, a threshold that is negative or NaN, a null output (needs_aa_dev included);
 * C2RT_ERR_UNSUPPORTED naming "strip_world" for opts->strip_world > 1. */
int c2rt_render_frames_adaptive_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames,
                                       const c2rt_render_opts *opts, float threshold, float *out_rgb_dev,
                                       uint8_t *needs_aa_dev, void *hip_stream);
/* The same into HOST memory: frames and flags are staged in the context's staging buffer on the context's own stream
 * and copied back once each (`needs_aa` is nullable here); blocks until they are there.  `stop_flag` is polled once,
 * before the launches; C2RT_ERR_CANCELLED leaves the outputs untouched. */
int c2rt_render_frames_adaptive(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames,
                                const c2rt_render_opts *opts, float threshold, float *out_rgb, uint8_t *needs_aa,
                                const volatile uint8_t *stop_flag);

/* An anti-aliased animation in one call: c2rt_render_frames_adaptive_device with a pose per frame, as
 * c2rt_render_frames_posed_device is to c2rt_render_frames_device.  Frame i and its flags hold exactly the bits
 * c2rt_update_scene(&poses[i]) followed by c2rt_render_frame_adaptive_device(&cams[i]) writes, each pose relative to the
 * context's scene as it is; the context's scene is unchanged by the call.  Frame i's refinement traces frame i's node
 * and light tables, the copies that travel behind the batch's table.  Enqueue order, blocking, streams and scratch: as
 * c2rt_render_frames_adaptive_device, the one-tap batch being c2rt_render_frames_posed_device's (plane-instance groups
 * included).  Statuses: those of c2rt_render_frames_adaptive_device in its order, then null `poses`:
 * C2RT_ERR_INVALID_ARG, then those of c2rt_update_scene for every poses[i], with "frame i: " in front of the message. */
int c2rt_render_frames_posed_adaptive_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses,
                                             uint32_t n_frames, const c2rt_render_opts *opts, float threshold,
                                             float *out_rgb_dev, uint8_t *needs_aa_dev, void *hip_stream);
/* The same into HOST memory, as c2rt_render_frames_adaptive is to c2rt_render_frames_adaptive_device. */
int c2rt_render_frames_posed_adaptive(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses,
                                      uint32_t n_frames, const c2rt_render_opts *opts, float threshold, float *out_rgb,
                                      uint8_t *needs_aa, const volatile uint8_t *stop_flag);

/* ---- sample tables: N-tap supersampled frames, whole and adaptive ------------ */

/* The table travels as a kernel argument behind the frame's parameter block (no copy, no scratch slot), which is what
 * bounds it; a 4x4 grid is the largest regular pattern under the cap. */
#define C2RT_MAX_SAMPLE_TAPS 16          /* C2RT_ERR_LIMIT beyond */

typedef struct c2rt_tap_table {          /* 264 bytes */
    uint32_t n;                          /* 1 .. C2RT_MAX_SAMPLE_TAPS */
    uint32_t reserved;                   /* must be 0 */
    double   offset[C2RT_MAX_SAMPLE_TAPS][2];   /* tap s samples the screen point (x + offset[s][0], y + offset[s][1]);
                                                    entries s >= n are not read */
} c2rt_tap_table;

/* A frame whose pixels average the caller's taps, for a pinhole, mono camera.  A composition of existing calls: for the
 * pixel (x, y) (frame row and column; strips as in c2rt_render_hits),
 *   for s in 0 .. n-1: c_s = the colour c2rt_trace_rays computes for the ray through the screen point
 *                            ((double)x + offset[s][0], (double)y + offset[s][1]) — Camera.getScreenRay and raytrace()'s
 *                            normalisation, the frames' own operations;
 *   accum = c_0; accum = accum + c_s for s = 1 .. n-1 (fp32, per channel, in tap order, no contraction);
 *   out = n > 1 ? accum / (float)n : accum  (Color / float: a division, not a reciprocal).
 * These are the frame kernels' statements, so bit for bit: the reference's five taps ({0,0}, {.3,.3}, {.6,0}, {0,.6},
 * {.6,.6}) give the C2RT_TAPS_REF5 frame of c2rt_render_frame_device, their first four the C2RT_TAPS_4 frame, and
 * {(0,0)} the C2RT_TAPS_1 frame and the hit planes' rgb.  Offsets may be negative or exceed 1 (the tap then samples a
 * neighbour's area).  opts->taps must be a valid mode and is otherwise ignored; opts->seed is ignored.  Strips give
 * compact rows, c2rt_local_rows(opts) of them; on a multi-device context the call runs on the lead device; after
 * c2rt_update_scene it sees the posed scene.
 *
 * The _device variant is ONE kernel on `hip_stream` (a hipStream_t, NULL = default stream): no host sync, no event left
 * in the queue, no scratch slot, no reference kept to the stream.
 *
 * Statuses, all decided before anything is enqueued or written, in this order: those of a frame call, in
 * c2rt_render_hits' order (null context, camera or options: C2RT_ERR_INVALID_ARG; no scene: C2RT_ERR_NO_SCENE; bad size
 * / tap mode / strip rank); null `taps`: C2RT_ERR_INVALID_ARG; n == 0: C2RT_ERR_INVALID_ARG; n > C2RT_MAX_SAMPLE_TAPS:
 * C2RT_ERR_LIMIT; reserved != 0: C2RT_ERR_INVALID_ARG; a NaN or infinite offset among the first n:
 * C2RT_ERR_INVALID_ARG, the message naming the tap; null output: C2RT_ERR_INVALID_ARG; C2RT_ERR_UNSUPPORTED with the
 * cause named in c2rt_last_error for cam->dof ("depth of field"), cam->stereo_separation != 0 ("stereo"),
 * opts->count_rays ("count_rays") and opts->prepass_bucket ("prepass_bucket"). */
int c2rt_render_frame_taps_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                                  const c2rt_tap_table *taps, float *out_rgb_dev, void *hip_stream);
/* The same into HOST memory: through the context's staging buffer on the context's own stream, in chunks of whole rows of
 * at most 2^18 pixels (12 B per pixel); blocks until the frame is there. */
int c2rt_render_frame_taps(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                           const c2rt_tap_table *taps, float *out_rgb);

/* c2rt_render_frame_adaptive_device with step 3 generalised to the caller's table.  Steps 1 and 2 are that call's: the
 * one-tap frame from the frame path with taps = 1, the detection kernel and its mask.  Step 3, for the flagged pixels
 * only: accum = out[y][x]; accum += c_s for s = 1 .. n-1 in that order (c_s as above); out[y][x] = accum / (float)n.
 * The call requires n >= 2 and offset[0] == (0, 0), so a flagged pixel holds the bits of c2rt_render_frame_taps for the
 * same table and an unflagged pixel the bits of the C2RT_TAPS_1 frame; with the reference's five taps, frame and mask
 * are the bits of c2rt_render_frame_adaptive_device.  opts->taps must be a valid mode and is otherwise ignored.
 * Enqueue order, streams, the required needs_aa_dev: as c2rt_render_frame_adaptive_device, with this refinement kernel
 * in the place of its own.
 *
 * Statuses, all decided before anything is enqueued or written, in this order: those of a frame call;
 * C2RT_ERR_INVALID_ARG (C2RT_ERR_LIMIT for n > C2RT_MAX_SAMPLE_TAPS) for a bad table as above, then for n < 2, for
 * offset[0] != (0, 0), for a threshold that is negative or NaN, for a null output (needs_aa_dev included); then the
 * C2RT_ERR_UNSUPPORTED causes of c2rt_render_frame_adaptive_device, "strip_world" and "multi-device" among them. */
int c2rt_render_frame_adaptive_taps_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                                           const c2rt_tap_table *taps, float threshold,
                                           float *out_rgb_dev, uint8_t *needs_aa_dev, void *hip_stream);
/* The same into HOST memory, as c2rt_render_frame_adaptive is to c2rt_render_frame_adaptive_device: `needs_aa` is
 * nullable here; `stop_flag` is polled once, before the launches; C2RT_ERR_CANCELLED leaves the outputs untouched. */
int c2rt_render_frame_adaptive_taps(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                                    const c2rt_tap_table *taps, float threshold,
                                    float *out_rgb, uint8_t *needs_aa, const volatile uint8_t *stop_flag);

/* Rank-0 side of the multi-GPU gather: `gathered_dev` holds `world`
 * consecutive compact strip buffers (rank-major, as ncclGather leaves them);
 * writes the de-interleaved full frame to `frame_dev`.  Both device
 * pointers; enqueued on `hip_stream`. */
int c2rt_deinterleave_strips(c2rt_ctx *ctx, const float *gathered_dev,
                             float *frame_dev, uint32_t width, uint32_t height,
                             uint32_t strip_height, uint32_t world,
                             void *hip_stream);

/* Downstream display encode, fused on device (rt/color.d:154-162,194-228,
 * gui/sdl2_gui.d:139-155): float RGB -> 0x00RRGGBB via the reference's
 * 4097-entry sRGB table (including its 12.02 quirk). */
int c2rt_encode_rgb32(c2rt_ctx *ctx, const float *frame_dev, uint32_t *out_dev,
                      uint64_t n_pixels, void *hip_stream);

/* The frame in display format: render + the encode above on the device, then
 * 4 B/pixel (instead of 12) over PCIe into the caller's host buffer — what
 * SDL2Gui.draw (gui/sdl2_gui.d:139-155) computes per pixel on the CPU from the
 * float frame.  Same blocking / stop-flag behaviour as c2rt_render_frame. */
int c2rt_render_frame_rgb32(c2rt_ctx *ctx, const c2rt_camera_frame *cam,
                            const c2rt_render_opts *opts, uint32_t *out_rgb32,
                            const volatile uint8_t *stop_flag);

/* c2rt_deinterleave_strips for packed RGB32 strips (one 32-bit word per pixel). */
int c2rt_deinterleave_strips_rgb32(c2rt_ctx *ctx, const uint32_t *gathered_dev,
                                   uint32_t *frame_dev, uint32_t width, uint32_t height,
                                   uint32_t strip_height, uint32_t world, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* C2RT_H */

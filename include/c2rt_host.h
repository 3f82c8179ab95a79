/*
 * c2rt_host.h — C view of the host-side mirror of the reference's
 * Scene / Camera / Renderer API (C++ implementation in
 * chess2rt_amd/csrc/host/).  The reference is D and cannot be compiled in
 * the build environment, so the host side that would normally stay in D is
 * restated in C++ above the C ABI of c2rt.h; these wrappers let the Python
 * test driver and bench.py reach it through ctypes.
 *
 * Mirrors (paths relative to /root/reference/source):
 *   parseSceneFromFile   rt/scene_loader.d:20-41
 *   Scene.beginFrame     rt/scene.d:55-58 -> Camera.beginFrame rt/camera.d:77-117
 *   updateToWindowSize   gui/raytracer_demo.d:126-143 (frame-size override)
 *   Renderer.renderRT    rt/renderer.d:83-192
 *   renderSceneAsync     rt/renderer.d:23-44
 *   renderPixel          rt/renderer.d:46-57
 *   Camera.move/rotate   rt/camera.d:181-229
 *   Transform            rt/transform.d:24-63
 *   Bitmap.loadImage     rt/bitmap.d:67-80, imageio/bmp.d:60-193
 *   Bitmap.saveImage     rt/bitmap.d:84-103, imageio/bmp.d:195-237
 */
#ifndef C2RT_HOST_H
#define C2RT_HOST_H

#include "c2rt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct c2rt_host_scene c2rt_host_scene;

/* GlobalSettings as parsed (rt/global_settings.d:5-32). */
typedef struct c2rt_host_settings {
    uint32_t frame_width, frame_height;
    uint32_t fullscreen, allow_resize, dynamic_aspect_ratio, interactive;
    uint32_t bucket_size, thread_count;
    uint32_t prepass_enabled, prepass_only, gi_enabled, aa_enabled;
    double aa_threshold;
    uint32_t paths_per_pixel, max_trace_depth;
    float ambient[3];
    uint32_t debug_enabled;
} c2rt_host_settings;

/* Camera fields (rt/camera.d:29-45). */
typedef struct c2rt_host_camera {
    uint64_t frame_width, frame_height;
    double aspect;
    double pos[3];
    double yaw, pitch, roll, fov;
    double focal_plane_dist, f_number, disc_multiplier;
    uint32_t dof;
    uint64_t num_samples;
    double stereo_separation;
} c2rt_host_camera;

/* parseSceneFromFile.  On failure returns C2RT_ERR_IO (SceneNotFoundException)
 * or C2RT_ERR_PARSE (InvalidSceneException, EntityWithDuplicateName, ...) and
 * writes a message to `err` (nullable). */
int c2rt_host_scene_load(const char *path, c2rt_host_scene **out, char *err, size_t err_len);
void c2rt_host_scene_free(c2rt_host_scene *scene);
const char *c2rt_host_scene_name(const c2rt_host_scene *scene);

/* The flat tables for c2rt_upload_scene; owned by the scene, valid until it
 * is freed or mutated. */
const c2rt_scene_desc *c2rt_host_scene_desc(c2rt_host_scene *scene);

void c2rt_host_scene_get_settings(const c2rt_host_scene *scene, c2rt_host_settings *out);
void c2rt_host_scene_get_camera(const c2rt_host_scene *scene, c2rt_host_camera *out);
void c2rt_host_scene_set_camera(c2rt_host_scene *scene, const c2rt_host_camera *in);

/* settings.frameWidth/Height := w,h and camera.setFrameSize(w,h), as
 * RTDemo.updateToWindowSize does with dynamicAspectRatio. */
void c2rt_host_scene_set_frame_size(c2rt_host_scene *scene, uint32_t width, uint32_t height);
void c2rt_host_scene_set_aa(c2rt_host_scene *scene, uint32_t aa_enabled);
void c2rt_host_scene_set_dof(c2rt_host_scene *scene, uint32_t dof);

/* Scene.beginFrame: computes the camera frame for the current settings. */
void c2rt_host_scene_begin_frame(c2rt_host_scene *scene, c2rt_camera_frame *out);
/* Camera.move / Camera.rotate (need a beginFrame before move). */
void c2rt_host_camera_move(c2rt_host_scene *scene, double dx, double dy, double dz);
void c2rt_host_camera_rotate(c2rt_host_scene *scene, double dyaw, double droll, double dpitch);

/* Renderer.renderRT through the GPU library: uploads the scene if `ctx` has
 * none from this scene yet, beginFrame, taps from AAEnabled, blocking.
 * `out_rgb` is frameWidth*frameHeight*3 floats (Image!Color). */
int c2rt_host_render_rt(c2rt_ctx *ctx, c2rt_host_scene *scene, float *out_rgb,
                        const volatile uint8_t *stop_flag);
/* renderSceneAsync: beginFrame on the caller's thread, then one render
 * thread; `*is_rendering` is cleared when the frame is complete,
 * `needs_rendering` is the stop request. */
int c2rt_host_render_scene_async(c2rt_ctx *ctx, c2rt_host_scene *scene, float *out_rgb,
                                 volatile uint8_t *is_rendering,
                                 const volatile uint8_t *needs_rendering);
/* joins the render thread of the last async call (test helper) */
int c2rt_host_render_wait(c2rt_host_scene *scene);
/* renderPixel */
int c2rt_host_render_pixel(c2rt_ctx *ctx, c2rt_host_scene *scene, int x, int y,
                           c2rt_trace_result *out);

/* The hit planes of the scene's own camera at its frame size (c2rt_render_hits: one plane per field of the probe's
 * record, frame_height x frame_width, host pointers, every one nullable): uploads the scene if needed and calls
 * beginFrame, as c2rt_host_render_pixel does.  A scene whose camera has depth of field or stereo is refused with
 * C2RT_ERR_UNSUPPORTED (c2rt_last_error names the cause); the AA setting does not matter (one sample per pixel). */
int c2rt_host_render_hits(c2rt_ctx *ctx, c2rt_host_scene *scene, const c2rt_hit_planes *planes);

/* The hit layers of the scene's own camera at its frame size (c2rt_render_hit_layers: layer k's slice of a plane
 * k * frame_height * frame_width * components elements behind its pointer, `count` frame_height x frame_width bytes,
 * host pointers, every one nullable): to c2rt_host_render_hits what that call is to c2rt_render_hits. */
int c2rt_host_render_hit_layers(c2rt_ctx *ctx, c2rt_host_scene *scene, uint32_t max_layers,
                                const c2rt_hit_planes *planes, uint8_t *count);

/* The shading planes of the scene's own camera at its frame size (c2rt_render_shading: frame_height x frame_width
 * samples per plane, host pointers, every one nullable): as c2rt_host_render_hits is to c2rt_render_hits. */
int c2rt_host_render_shading(c2rt_ctx *ctx, c2rt_host_scene *scene, const c2rt_shade_planes *planes);

/* The occlusion planes of the scene's own camera at its frame size (c2rt_render_occlusion: frame_height x frame_width
 * samples per plane, host pointers, every one nullable; `occ` as there): as c2rt_host_render_hits is to c2rt_render_hits. */
int c2rt_host_render_occlusion(c2rt_ctx *ctx, c2rt_host_scene *scene, const c2rt_occlusion_opts *occ,
                               const c2rt_occlusion_planes *planes);

/* The gather planes of the scene's own camera at its frame size (c2rt_render_gather: frame_height x frame_width samples
 * per plane, host pointers, every one nullable; `g` as there): as c2rt_host_render_hits is to c2rt_render_hits. */
int c2rt_host_render_gather(c2rt_ctx *ctx, c2rt_host_scene *scene, const c2rt_gather_opts *g, const c2rt_gather_planes *planes);

/* The path planes of the scene's own camera at its frame size (c2rt_render_paths: frame_height x frame_width samples
 * per plane, host pointers, every one nullable; `g` as there — the scene's own pathsPerPixel and maxTraceDepth are in
 * c2rt_host_settings): as c2rt_host_render_hits is to c2rt_render_hits. */
int c2rt_host_render_paths(c2rt_ctx *ctx, c2rt_host_scene *scene, const c2rt_path_opts *g, const c2rt_path_planes *planes);

/* The denoised global-illumination frame of the scene's own camera at its frame size (c2rt_render_paths_denoised:
 * `out_rgb` frame_height x frame_width x 3 floats; `g` and `d` as there, d->width / d->height the scene's frame size): as
 * c2rt_host_render_hits is to c2rt_render_hits. */
int c2rt_host_render_paths_denoised(c2rt_ctx *ctx, c2rt_host_scene *scene, const c2rt_path_opts *g, const c2rt_denoise_opts *d, float *out_rgb);

/* Renderer.renderRT with adaptive anti-aliasing (c2rt_render_frame_adaptive) for the scene's own camera at its frame
 * size, with the reference's threshold (C2RT_AA_THRESHOLD_REF) and C2RT_TAPS_REF5 whatever the AA setting: uploads the
 * scene if needed and calls beginFrame.  `out_rgb`: frameWidth * frameHeight * 3 floats; `needs_aa` (nullable):
 * frameWidth * frameHeight bytes.  Depth of field and stereo are refused with C2RT_ERR_UNSUPPORTED. */
int c2rt_host_render_rt_adaptive(c2rt_ctx *ctx, c2rt_host_scene *scene, float *out_rgb, uint8_t *needs_aa);

/* The scene's own camera at its frame size through a caller's tap table: c2rt_render_frame_taps (every pixel the average
 * of the table's taps) and c2rt_render_frame_adaptive_taps at the reference's threshold (taps 1 .. n-1 on the flagged
 * pixels only; `needs_aa` nullable).  Both upload the scene if needed and call beginFrame; the table, the outputs and the
 * camera are judged by those calls. */
int c2rt_host_render_rt_taps(c2rt_ctx *ctx, c2rt_host_scene *scene, const c2rt_tap_table *taps, float *out_rgb);
int c2rt_host_render_rt_adaptive_taps(c2rt_ctx *ctx, c2rt_host_scene *scene, const c2rt_tap_table *taps, float *out_rgb,
                                      uint8_t *needs_aa);

/* ---- moving a node or a light of a loaded scene ----------------------------- */

/* Index of the named node / light in the flat tables (and in a c2rt_scene_pose); -1: no such name. */
int c2rt_host_scene_node_index(const c2rt_host_scene *scene, const char *node);
int c2rt_host_scene_light_index(const c2rt_host_scene *scene, const char *light);

/* The named node's Transform (rt/node.d:9, rt/transform.d:11-14) with the reference's own verbs: reset (:24-29), scale
 * (:31-39), rotate (:41-50, the real one: see c2rt_host_transform_rotate), translate (:52-55); _get / _set hand the 30
 * doubles of c2rt_scene_desc::node_transform over whole.  Each call patches the host object and its flat view in place
 * (c2rt_host_scene_desc stays valid).  If `ctx` (nullable) still holds this scene's own upload, the call also pushes
 * the change with one c2rt_update_scene on the default stream and the generation stays this scene's: the next render
 * shows the moved node without a re-upload.  Without a context, with a context that has moved on to another scene, or
 * after a refused update, the next render through this scene re-uploads, as it always did.  C2RT_ERR_INVALID_ARG: no
 * such node; otherwise c2rt_update_scene's status. */
int c2rt_host_node_transform_get(const c2rt_host_scene *scene, const char *node, double t[30]);
int c2rt_host_node_transform_set(c2rt_ctx *ctx, c2rt_host_scene *scene, const char *node, const double t[30]);
int c2rt_host_node_transform_reset(c2rt_ctx *ctx, c2rt_host_scene *scene, const char *node);
int c2rt_host_node_transform_scale(c2rt_ctx *ctx, c2rt_host_scene *scene, const char *node, double x, double y, double z);
int c2rt_host_node_transform_rotate(c2rt_ctx *ctx, c2rt_host_scene *scene, const char *node, double yaw, double pitch, double roll);
int c2rt_host_node_transform_translate(c2rt_ctx *ctx, c2rt_host_scene *scene, const char *node, const double v[3]);
/* The named light's PointLight.pos, Light.lightColor and Light.lightPower (rt/light.d); a null pointer leaves that
 * field as it is.  `ctx` as above. */
int c2rt_host_light_set(c2rt_ctx *ctx, c2rt_host_scene *scene, const char *light, const double *pos, const float *color,
                        const float *power);

/* loadBmpImage!Color: malloc'd width*height*3 floats (free with
 * c2rt_host_free); y = 0 is the top row.  No gamma decode. */
int c2rt_host_bmp_decode(const uint8_t *bytes, size_t len, uint32_t *width, uint32_t *height,
                         float **out_rgb);
/* BitmapTexture gamma step (rt/texture.d:137-141, rt/bitmap.d:116-136). */
void c2rt_host_texture_gamma(float *texels, size_t n_floats, float assumed_gamma);
/* Color.toRGB32 + saveBmp 24-bpp: malloc'd file image. */
int c2rt_host_bmp_encode(const float *rgb, uint32_t width, uint32_t height, uint8_t **out_bytes,
                         size_t *out_len);
uint32_t c2rt_host_color_to_rgb32(const float rgb[3]);
void c2rt_host_free(void *p);

/* Transform (rt/transform.d:24-63) as the loader's mirror evaluates it.  `t` holds transform[9],
 * inverseTransform[9], transposedInverse[9] (row-major) and offset[3] — the layout of
 * c2rt_scene_desc::node_transform.  The REAL rotate (Rx(pitch) * Ry(yaw) * Rz(roll), :41-50) is reachable only
 * here: the scene loader's "rotate" key scales (reference bug). */
void c2rt_host_transform_reset(double t[30]);
void c2rt_host_transform_scale(double t[30], double x, double y, double z);
void c2rt_host_transform_rotate(double t[30], double yaw, double pitch, double roll);
void c2rt_host_transform_translate(double t[30], const double v[3]);
/* point(P) = mul(P, transform) + offset (:57-63) */
void c2rt_host_transform_point(const double t[30], const double p[3], double out[3]);

#ifdef __cplusplus
}
#endif
#endif

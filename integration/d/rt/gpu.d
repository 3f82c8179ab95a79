/**
 * rt.gpu — D-side binding of libc2rt.so (include/c2rt.h) for Chess2RT.
 *
 * WRITTEN, NOT COMPILED: the build environment of this repository has no D
 * toolchain (no dmd / ldc2 / gdc / dub), so this file could not be compiled
 * or run.  The identical boundary is exercised from C++
 * (chess2rt_amd/csrc/host/host_api.cpp + scene.cpp: `Scene::flatten`,
 * `Renderer::renderRT`) and from Python (chess2rt_amd/_abi.py), which is
 * what the tests use.  Drop this file into `source/rt/`, add `libs "c2rt"`
 * to dub.sdl and replace the lambda body in rt/renderer.d:36-37 as shown at
 * the bottom.
 *
 * Access note: Camera keeps upLeft/upRight/downLeft/frontDir/rightDir/upDir,
 * Sphere/CsgOp/BitmapTexture/Transform keep their fields `private` or
 * `protected` (rt/camera.d:47-53, rt/geometry.d:75-79,253-257,
 * rt/texture.d:149-161, rt/transform.d:11-14).  D's `private` is
 * module-level, so either move `flatten` pieces into those modules or relax
 * the attributes to `package`; the code below assumes `package`.
 */
module rt.gpu;

import core.atomic : atomicStore;
import std.exception : enforce;
import std.string : fromStringz;

import imageio.image : Image;
import rt.camera, rt.color, rt.geometry, rt.light, rt.node, rt.scene, rt.shader, rt.texture, rt.importedtypes;

extern (C) nothrow @nogc
{
    struct c2rt_ctx;

    enum : int { C2RT_OK = 0, C2RT_ERR_CANCELLED = 7 }
    enum : int { GEOM_PLANE, GEOM_SPHERE, GEOM_CUBE, GEOM_CSG_UNION, GEOM_CSG_INTER, GEOM_CSG_DIFF }
    enum : int { SHADER_LAMBERT, SHADER_PHONG }
    enum : int { TEX_CHECKER, TEX_PROCEDURE2, TEX_BITMAP }

    struct c2rt_scene_desc
    {
        uint abi_version = 1;
        uint n_geoms; const(int)* geom_type; const(double)* geom_param; const(int)* geom_child;
        uint n_textures; const(int)* tex_type; const(float)* tex_color; const(double)* tex_param;
        const(float)* tex_scaling; const(uint)* tex_width; const(uint)* tex_height; const(ulong)* tex_offset;
        ulong n_texels; const(float)* texels;
        uint n_shaders; const(int)* shader_type; const(float)* shader_color; const(int)* shader_texture;
        const(double)* shader_exponent; const(float)* shader_strength;
        uint n_lights; const(int)* light_type; const(double)* light_pos; const(float)* light_color; const(float)* light_power;
        uint n_nodes; const(int)* node_geom; const(int)* node_shader; const(int)* node_bump; const(double)* node_transform;
        float[3] ambient; uint max_trace_depth; uint gi_enabled;
    }

    struct c2rt_camera_frame
    {
        double[3] pos, up_left, up_right, down_left, right_dir, up_dir, front_dir;
        double frame_width, frame_height;
        uint dof, num_samples;
        double focal_plane_dist, disc_multiplier, stereo_separation;
    }

    struct c2rt_render_opts
    {
        uint width, height, taps, strip_height, strip_rank, strip_world;
        ulong seed;
        uint count_rays, prepass_bucket;
    }

    struct c2rt_trace_result
    {
        float[3] color; int closest_node, leaf_geom;
        double[3] p, normal; double dist, u, v; double[3] ray_orig, ray_dir;
    }

    int c2rt_init(int device, c2rt_ctx** outCtx);
    int c2rt_init_multi(int device_count_or_0, const(int)* device_ids, c2rt_ctx** outCtx);
    int c2rt_device_count(const c2rt_ctx*);
    ulong c2rt_scene_generation(const c2rt_ctx*);
    void c2rt_destroy(c2rt_ctx*);
    const(char)* c2rt_last_error(const c2rt_ctx*);
    int c2rt_upload_scene(c2rt_ctx*, const c2rt_scene_desc*);
    int c2rt_render_frame(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, float* out_rgb,
                          const shared(ubyte)* stop_flag);
    int c2rt_pin_host_buffer(c2rt_ctx*, float* out_rgb, size_t bytes);
    int c2rt_unpin_host_buffer(c2rt_ctx*, float* out_rgb);
    int c2rt_render_pixel(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, int x, int y,
                          c2rt_trace_result*);
    /// display words (Color.toRGB32, encoded in the render kernel) straight into `screen`'s uint twin: what
    /// SDL2Gui.draw (gui/sdl2_gui.d:139-155) computes per pixel on the CPU today
    int c2rt_render_frame_rgb32(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, uint* out_rgb32,
                                const shared(ubyte)* stop_flag);
    /// tiles rendered a second time through the IEEE divide / sqrt path (a cost indicator; 0 on sane scenes)
    int c2rt_get_exact_redos(c2rt_ctx*, ulong* outCount);
    /// ground-only tiles handed from the short fp64 chain back to the full one (a cost indicator)
    int c2rt_get_ground_bails(c2rt_ctx*, ulong* outCount);
    int c2rt_get_sphere_bails(c2rt_ctx*, ulong* outCount);
    /// many cameras, one scene, one call: frame i at out + i * local_rows * width * 3 floats, the bits of the
    /// single-frame calls; no depth of field / stereo / counted / preview frames (C2RT_ERR_UNSUPPORTED)
    enum C2RT_MAX_BATCH_FRAMES = 256;
    int c2rt_render_frames_device(c2rt_ctx*, const c2rt_camera_frame* cams, uint nFrames, const c2rt_render_opts*,
                                  float* out_rgb_dev, void* hip_stream);
    int c2rt_render_frames(c2rt_ctx*, const c2rt_camera_frame* cams, uint nFrames, const c2rt_render_opts*,
                           float* out_rgb, const shared(ubyte)* stop_flag);
    /// move nodes and lights of the uploaded scene without re-uploading it: node_transform is [n_nodes][30] in the
    /// layout of c2rt_scene_desc.node_transform; the copies are ordered on hip_stream, the generation stays
    struct c2rt_scene_pose {
        uint n_nodes; const(uint)* node_index; const(double)* node_transform;
        uint n_lights; const(uint)* light_index; const(double)* light_pos; const(float)* light_color; const(float)* light_power;
    }
    int c2rt_update_scene(c2rt_ctx*, const c2rt_scene_pose* pose, void* hip_stream);
    /// an animation in one call: frame i is the current scene under poses[i], seen through cams[i]
    int c2rt_render_frames_posed_device(c2rt_ctx*, const c2rt_camera_frame* cams, const c2rt_scene_pose* poses, uint nFrames,
                                        const c2rt_render_opts*, float* out_rgb_dev, void* hip_stream);
    int c2rt_render_frames_posed(c2rt_ctx*, const c2rt_camera_frame* cams, const c2rt_scene_pose* poses, uint nFrames,
                                 const c2rt_render_opts*, float* out_rgb, const shared(ubyte)* stop_flag);
    /// ray queries: Renderer.trace (rt/renderer.d:325-376) and Scene.testVisibility (rt/scene.d:62-78) for the
    /// caller's own rays, one per GPU lane; `dir` is used as given (trace() does not normalise); hits / rgb nullable,
    /// not both; Vector is three doubles, so a Ray's orig and dir map onto c2rt_ray as they stand
    enum C2RT_MAX_RAYS = 1u << 28;
    struct c2rt_ray     { double[3] orig, dir; }
    struct c2rt_segment { double[3] from, to; }
    struct c2rt_ray_hit { int closest_node, leaf_geom; double dist, u, v; double[3] p, normal; }
    int c2rt_trace_rays_device(c2rt_ctx*, const c2rt_ray* rays_dev, ulong n, c2rt_ray_hit* hits_dev, float* rgb_dev,
                               void* hip_stream);
    int c2rt_trace_rays(c2rt_ctx*, const c2rt_ray* rays, ulong n, c2rt_ray_hit* hits, float* rgb);
    int c2rt_test_visibility_device(c2rt_ctx*, const c2rt_segment* seg_dev, ulong n, ubyte* visible_dev,
                                    void* hip_stream);
    int c2rt_test_visibility(c2rt_ctx*, const c2rt_segment* seg, ulong n, ubyte* visible);
    /// hit planes: renderPixel's TraceResult for every pixel of a frame in one call, one plane per field, row-major
    /// local_rows x width; every pointer nullable (a null plane is neither computed nor stored), at least one given;
    /// no depth of field / stereo / counted / preview frames (C2RT_ERR_UNSUPPORTED)
    struct c2rt_hit_planes
    {
        int* node, leaf;            /// closest node / leaf geometry, -1 without a hit
        double* dist;               /// 1e99 without a hit
        double* uv, p, normal;      /// [2], [3], [3] per pixel; 0 without a hit
        float* rgb;                 /// [3] per pixel: the one-tap frame
    }
    int c2rt_render_hits_device(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*,
                                const c2rt_hit_planes* planes_dev, void* hip_stream);
    int c2rt_render_hits(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_hit_planes* planes_host);
    /// hit planes of a batch / of a posed animation in one launch: frame i's slice of a plane starts
    /// i * local_rows * W * components elements behind the plane's pointer (no padding) and holds the bits of the
    /// single-frame call (after c2rt_update_scene(&poses[i]) for the posed calls; the context's scene is unchanged)
    int c2rt_render_frames_hits_device(c2rt_ctx*, const c2rt_camera_frame* cams, uint nFrames, const c2rt_render_opts*,
                                       const c2rt_hit_planes* planes_dev, void* hip_stream);
    int c2rt_render_frames_hits(c2rt_ctx*, const c2rt_camera_frame* cams, uint nFrames, const c2rt_render_opts*,
                                const c2rt_hit_planes* planes_host);
    int c2rt_render_frames_posed_hits_device(c2rt_ctx*, const c2rt_camera_frame* cams, const c2rt_scene_pose* poses,
                                             uint nFrames, const c2rt_render_opts*, const c2rt_hit_planes* planes_dev,
                                             void* hip_stream);
    int c2rt_render_frames_posed_hits(c2rt_ctx*, const c2rt_camera_frame* cams, const c2rt_scene_pose* poses, uint nFrames,
                                      const c2rt_render_opts*, const c2rt_hit_planes* planes_host);
    /// hit layers: every surface along a ray / behind a pixel, in order, in one launch (findAllIntersections,
    /// rt/geometry.d:271-290, over the scene's trace); layer-major outputs (layer k of ray i at k * n + i, layer k's slice
    /// of a plane k * local_rows * W * components elements behind its pointer), count = hits stored per ray / pixel;
    /// slot k means something for k <= count only; every output nullable, not all
    enum C2RT_MAX_HIT_LAYERS = 16;
    int c2rt_trace_rays_layers_device(c2rt_ctx*, const c2rt_ray* rays_dev, ulong n, uint max_layers, c2rt_ray_hit* hits_dev,
                                      float* rgb_dev, ubyte* count_dev, void* hip_stream);
    int c2rt_trace_rays_layers(c2rt_ctx*, const c2rt_ray* rays, ulong n, uint max_layers, c2rt_ray_hit* hits, float* rgb,
                               ubyte* count);
    int c2rt_render_hit_layers_device(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, uint max_layers,
                                      const c2rt_hit_planes* planes_dev, ubyte* count_dev, void* hip_stream);
    int c2rt_render_hit_layers(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, uint max_layers,
                               const c2rt_hit_planes* planes_host, ubyte* count_host);
    /// shading planes: the terms of the closest node's shade() of one sample, one nullable plane each; on a hit
    /// rgb == albedo * light (+ specular for Phong) bit for bit, and rgb / node are the hit planes'
    struct c2rt_shade_planes
    {
        int* node;                  /// closest node, -1: no hit
        float* albedo, light;       /// [3] per sample: diffuseColor, lightContrib
        float* specular;            /// [3] per sample: Phong's specular; +0 for a Lambert node
        uint* visible;              /// bit l: light l < 32 passed intensity() != 0 && testVisibility
        float* rgb;                 /// [3] per sample: shade's return value
    }
    int c2rt_render_shading_device(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*,
                                   const c2rt_shade_planes* planes_dev, void* hip_stream);
    int c2rt_render_shading(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_shade_planes* planes_host);
    int c2rt_trace_rays_shading_device(c2rt_ctx*, const c2rt_ray* rays_dev, ulong n, const c2rt_shade_planes* planes_dev,
                                       void* hip_stream);
    int c2rt_trace_rays_shading(c2rt_ctx*, const c2rt_ray* rays, ulong n, const c2rt_shade_planes* planes_host);
    /// occlusion planes: `samples` segments of length `radius` from p + N * 1e-6 over hemisphereSample(N) of the closest
    /// hit, each answered by testVisibility; sample index: frame row * W + column, or the ray's index (include/c2rt.h)
    enum uint C2RT_MAX_OCCLUSION_SAMPLES = 64;
    struct c2rt_occlusion_opts
    {
        double radius;              /// length of every segment; finite, > 0
        ulong seed;                 /// counter-RNG seed
        uint samples;               /// K: 1 .. C2RT_MAX_OCCLUSION_SAMPLES
        uint reserved;              /// must be 0
    }
    struct c2rt_occlusion_planes
    {
        int* node;                  /// closest node, -1: no hit
        ulong* open;                /// bit s < K: sample s's segment is unoccluded
        float* ao;                  /// popcount(open) / K
        double* bent;               /// [3] per sample: sum of the open samples' directions, not normalised
    }
    int c2rt_render_occlusion_device(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_occlusion_opts*,
                                     const c2rt_occlusion_planes* planes_dev, void* hip_stream);
    int c2rt_render_occlusion(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_occlusion_opts*,
                              const c2rt_occlusion_planes* planes_host);
    int c2rt_trace_rays_occlusion_device(c2rt_ctx*, const c2rt_ray* rays_dev, ulong n, const c2rt_occlusion_opts*,
                                         const c2rt_occlusion_planes* planes_dev, void* hip_stream);
    int c2rt_trace_rays_occlusion(c2rt_ctx*, const c2rt_ray* rays, ulong n, const c2rt_occlusion_opts*,
                                  const c2rt_occlusion_planes* planes_host);
    /// gather planes: `samples` rays from p + N * 1e-6 over hemisphereSample(N) of the closest hit (the occlusion planes'
    /// directions), each traced and shaded as c2rt_trace_rays does, weighted 2 cos and averaged (include/c2rt.h)
    enum uint C2RT_MAX_GATHER_SAMPLES = 64;
    struct c2rt_gather_opts
    {
        ulong seed;                 /// counter-RNG seed
        uint samples;               /// K: 1 .. C2RT_MAX_GATHER_SAMPLES
        uint reserved;              /// must be 0
    }
    struct c2rt_gather_planes
    {
        int* node;                  /// closest node, -1: no hit
        ulong* hits;                /// bit s < K: sample s's ray hit a node
        float* indirect;            /// [3] per sample: mean weighted colour arriving over the hemisphere
        float* bounce;              /// [3] per sample: albedo * indirect, what to add to the frame's colour
    }
    int c2rt_render_gather_device(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_gather_opts*,
                                  const c2rt_gather_planes* planes_dev, void* hip_stream);
    int c2rt_render_gather(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_gather_opts*,
                           const c2rt_gather_planes* planes_host);
    int c2rt_trace_rays_gather_device(c2rt_ctx*, const c2rt_ray* rays_dev, ulong n, const c2rt_gather_opts*,
                                      const c2rt_gather_planes* planes_dev, void* hip_stream);
    int c2rt_trace_rays_gather(c2rt_ctx*, const c2rt_ray* rays, ulong n, const c2rt_gather_opts*,
                               const c2rt_gather_planes* planes_host);
    /// path planes: `paths` paths of at most min(`bounces`, the scene's max_trace_depth) segments behind the closest hit,
    /// every vertex continued as Lambert.spawnRay continues it, every segment traced and shaded as c2rt_trace_rays does,
    /// weighted with the path's throughput and averaged: renderSampleGI's frame as `radiance` (include/c2rt.h)
    enum uint C2RT_MAX_PATHS = 64;
    enum uint C2RT_MAX_PATH_BOUNCES = 8;
    struct c2rt_path_opts
    {
        ulong seed;                 /// counter-RNG seed
        uint paths;                 /// P: 1 .. C2RT_MAX_PATHS
        uint bounces;               /// B: 1 .. C2RT_MAX_PATH_BOUNCES
    }
    struct c2rt_path_planes
    {
        int* node;                  /// closest node, -1: no hit
        uint* segments;             /// spawned segments that hit a node, over all paths and depths
        float* indirect;            /// [3] per sample: mean weighted light arriving at the hit, all depths
        float* bounce;              /// [3] per sample: albedo * indirect
        float* radiance;            /// [3] per sample: rgb + bounce, the global-illumination frame itself
    }
    int c2rt_render_paths_device(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_path_opts*,
                                 const c2rt_path_planes* planes_dev, void* hip_stream);
    int c2rt_render_paths(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_path_opts*,
                          const c2rt_path_planes* planes_host);
    int c2rt_trace_rays_paths_device(c2rt_ctx*, const c2rt_ray* rays_dev, ulong n, const c2rt_path_opts*,
                                     const c2rt_path_planes* planes_dev, void* hip_stream);
    int c2rt_trace_rays_paths(c2rt_ctx*, const c2rt_ray* rays, ulong n, const c2rt_path_opts*,
                              const c2rt_path_planes* planes_host);
    /// denoise: edge-aware a-trous filter (5x5 B3-spline, taps 2^l pixels apart at level l) of a Monte-Carlo plane, guided
    /// by the hit planes' node, normal and p; full-frame planes, fp32 arithmetic fixed by include/c2rt.h
    enum C2RT_MAX_DENOISE_LEVELS = 8;
    struct c2rt_denoise_guides
    {
        const(int)* node;           /// required: the hit planes' node, < 0: no hit
        const(double)* normal;      /// required: [3] per pixel
        const(double)* p;           /// required: [3] per pixel
        const(float)* albedo;       /// nullable: [channels] per pixel, multiplied into the result
        const(float)* base;         /// nullable: [channels] per pixel, added to the result
    }
    struct c2rt_denoise_opts
    {
        uint width, height;         /// the whole frame
        uint levels;                /// 0 .. C2RT_MAX_DENOISE_LEVELS
        uint channels;              /// 1 | 3
        uint normal_power_log2;     /// 0 .. 7
        float sigma_plane;          /// finite, > 0
        float sigma_colour;         /// finite, >= 0; 0: no colour term
        uint reserved;              /// 0
    }
    size_t c2rt_denoise_scratch_bytes(const c2rt_denoise_opts*);
    int c2rt_denoise_device(c2rt_ctx*, const c2rt_denoise_guides* guides_dev, const c2rt_denoise_opts*, const float* in_dev,
                            float* out_dev, void* scratch_dev, void* hip_stream);
    int c2rt_denoise(c2rt_ctx*, const c2rt_denoise_guides* guides_host, const c2rt_denoise_opts*, const float* in_, float* out_);
    int c2rt_render_paths_denoised(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_path_opts*,
                                   const c2rt_denoise_opts*, float* out_rgb);
    /// temporal accumulation: reproject the previous frame's history through the hit planes' p, fold the new sample into a
    /// running mean; full-frame planes, fp64 reprojection and fp32 gather fixed by include/c2rt.h
    enum C2RT_MAX_TEMPORAL_AGE = 65535;
    struct c2rt_temporal_opts
    {
        uint width, height;         /// the whole frame
        uint channels;              /// 1 | 3
        uint max_age;               /// 1 .. C2RT_MAX_TEMPORAL_AGE
        float min_normal_dot;       /// finite, 0 <= . < 1
        float max_plane_dist;       /// finite, > 0
        uint[2] reserved;           /// 0
    }
    struct c2rt_temporal_guides
    {
        const(int)* node;           /// the CURRENT frame's hit planes, all required
        const(double)* normal;      /// [3] per pixel
        const(double)* p;           /// [3] per pixel
    }
    struct c2rt_temporal_planes
    {
        float* colour;              /// nullable: [channels] per pixel, the accumulated plane
        float* variance;            /// nullable: temporal variance of the luminance
        uint* age;                  /// nullable: 0 miss, 1 no history, .. max_age
    }
    size_t c2rt_temporal_history_bytes(const c2rt_temporal_opts*);
    int c2rt_temporal_accumulate_device(c2rt_ctx*, const c2rt_camera_frame* prev_cam, const c2rt_temporal_guides* guides_dev,
                                        const c2rt_temporal_opts*, const float* in_dev, const void* history_prev_dev,
                                        void* history_out_dev, const c2rt_temporal_planes* planes_dev, void* hip_stream);
    int c2rt_temporal_accumulate(c2rt_ctx*, const c2rt_camera_frame* prev_cam, const c2rt_temporal_guides* guides_host,
                                 const c2rt_temporal_opts*, const float* in_, const void* history_prev, void* history_out,
                                 const c2rt_temporal_planes* planes_host);
    int c2rt_render_paths_sequence(c2rt_ctx*, const c2rt_camera_frame* cams, uint n_frames, const c2rt_render_opts*,
                                   const c2rt_path_opts*, const c2rt_temporal_opts*, const c2rt_denoise_opts*, float* out_rgb);
    /// variance-guided denoise: the a-trous filter with a luminance term scaled by the pixel's own standard deviation (the
    /// temporal planes' variance, filtered along; a spatial 7x7 estimate for pixels younger than min_age); fp32 arithmetic
    /// fixed by include/c2rt.h
    enum C2RT_MAX_VARIANCE_MIN_AGE = 64;
    struct c2rt_denoise_variance_opts
    {
        uint width, height;         /// the whole frame
        uint levels;                /// 0 .. C2RT_MAX_DENOISE_LEVELS
        uint channels;              /// 1 | 3
        uint normal_power_log2;     /// 0 .. 7
        float sigma_plane;          /// finite, > 0
        float sigma_lum;            /// finite, >= 0; 0: no luminance term
        float var_floor;            /// finite, > 0
        uint min_age;               /// 0 .. C2RT_MAX_VARIANCE_MIN_AGE; 0: no spatial estimate
        uint reserved;              /// 0
    }
    size_t c2rt_denoise_variance_scratch_bytes(const c2rt_denoise_variance_opts*);
    int c2rt_denoise_variance_device(c2rt_ctx*, const c2rt_denoise_guides* guides_dev, const c2rt_denoise_variance_opts*,
                                     const float* variance_dev, const uint* age_dev, const float* in_dev, float* out_dev,
                                     float* variance_out_dev, void* scratch_dev, void* hip_stream);
    int c2rt_denoise_variance(c2rt_ctx*, const c2rt_denoise_guides* guides_host, const c2rt_denoise_variance_opts*,
                              const float* variance, const uint* age, const float* in_, float* out_, float* variance_out);
    int c2rt_render_paths_sequence_variance(c2rt_ctx*, const c2rt_camera_frame* cams, uint n_frames, const c2rt_render_opts*,
                                            const c2rt_path_opts*, const c2rt_temporal_opts*, const c2rt_denoise_variance_opts*,
                                            float* out_rgb);
    /// the accumulation that follows moved nodes: per listed node the pose the history was made under and the pose of the
    /// current guides ([n][30] doubles, c2rt_scene_desc's node_transform layout); NULL or empty: c2rt_temporal_accumulate
    enum C2RT_MAX_MOTION_NODES = 16;
    struct c2rt_temporal_motion
    {
        uint n_nodes;               /// 0 .. C2RT_MAX_MOTION_NODES
        uint reserved;              /// 0
        const(uint)* node_index;    /// [n_nodes], distinct: the values the node plane holds
        const(double)* prev_transform;
        const(double)* cur_transform;
    }
    int c2rt_temporal_accumulate_motion_device(c2rt_ctx*, const c2rt_camera_frame* prev_cam, const c2rt_temporal_guides* guides_dev,
                                               const c2rt_temporal_opts*, const c2rt_temporal_motion*, const float* in_dev,
                                               const void* history_prev_dev, void* history_out_dev,
                                               const c2rt_temporal_planes* planes_dev, void* hip_stream);
    int c2rt_temporal_accumulate_motion(c2rt_ctx*, const c2rt_camera_frame* prev_cam, const c2rt_temporal_guides* guides_host,
                                        const c2rt_temporal_opts*, const c2rt_temporal_motion*, const float* in_,
                                        const void* history_prev, void* history_out, const c2rt_temporal_planes* planes_host);
    /// the two sequence calls with a pose per frame, each relative to the context's scene, which is unchanged afterwards
    int c2rt_render_paths_sequence_posed(c2rt_ctx*, const c2rt_camera_frame* cams, const c2rt_scene_pose* poses, uint n_frames,
                                         const c2rt_render_opts*, const c2rt_path_opts*, const c2rt_temporal_opts*,
                                         const c2rt_denoise_opts*, float* out_rgb);
    int c2rt_render_paths_sequence_posed_variance(c2rt_ctx*, const c2rt_camera_frame* cams, const c2rt_scene_pose* poses,
                                                  uint n_frames, const c2rt_render_opts*, const c2rt_path_opts*,
                                                  const c2rt_temporal_opts*, const c2rt_denoise_variance_opts*, float* out_rgb);
    /// counted path planes: the path planes with one byte per sample that says how many paths it gets, c = min(counts[i],
    /// paths); a sample at c >= 1 holds the bits of the uniform call at paths = c, a sample at 0 its node and primary colour.
    /// scratch_dev null: natural order, one kernel; else c2rt_paths_counted_scratch_bytes(samples) bytes, 16-byte aligned:
    /// the samples sorted by count ahead of the path kernel — the same bits (include/c2rt.h)
    size_t c2rt_paths_counted_scratch_bytes(ulong n_samples);
    int c2rt_render_paths_counted_device(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_path_opts*,
                                         const ubyte* counts_dev, const c2rt_path_planes* planes_dev, void* scratch_dev,
                                         void* hip_stream);
    int c2rt_render_paths_counted(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_path_opts*,
                                  const ubyte* counts, const c2rt_path_planes* planes_host);
    int c2rt_trace_rays_paths_counted_device(c2rt_ctx*, const c2rt_ray* rays_dev, ulong n, const c2rt_path_opts*,
                                             const ubyte* counts_dev, const c2rt_path_planes* planes_dev, void* scratch_dev,
                                             void* hip_stream);
    int c2rt_trace_rays_paths_counted(c2rt_ctx*, const c2rt_ray* rays, ulong n, const c2rt_path_opts*, const ubyte* counts,
                                      const c2rt_path_planes* planes_host);
    /// path counts: the counts plane of the NEXT frame from the previous history's variance at the point each pixel sees now
    /// (the accumulation's reprojection and gather without the fold); arithmetic fixed by include/c2rt.h
    struct c2rt_path_count_opts
    {
        uint min_paths;             /// 1 .. C2RT_MAX_PATHS
        uint max_paths;             /// min_paths .. C2RT_MAX_PATHS
        uint young_paths;           /// no history, or younger than min_age
        uint min_age;               /// 0 .. C2RT_MAX_TEMPORAL_AGE
        float paths_per_variance;   /// finite, > 0
        uint prev_paths;            /// the count behind every history pixel where prev_counts is null
        uint[2] reserved;           /// 0
    }
    int c2rt_path_counts_device(c2rt_ctx*, const c2rt_camera_frame* prev_cam, const c2rt_temporal_guides* guides_dev,
                                const c2rt_temporal_opts*, const c2rt_path_count_opts*, const void* history_prev_dev,
                                const ubyte* prev_counts_dev, ubyte* counts_dev, float* variance_dev, uint* age_dev,
                                void* hip_stream);
    int c2rt_path_counts(c2rt_ctx*, const c2rt_camera_frame* prev_cam, const c2rt_temporal_guides* guides_host,
                         const c2rt_temporal_opts*, const c2rt_path_count_opts*, const void* history_prev,
                         const ubyte* prev_counts, ubyte* counts, float* variance, uint* age);
    /// c2rt_render_paths_sequence_variance with the sampler in the loop: frame 0 at young_paths, frame i at the counts the
    /// rule makes of history i - 1
    int c2rt_render_paths_sequence_adaptive(c2rt_ctx*, const c2rt_camera_frame* cams, uint n_frames, const c2rt_render_opts*,
                                            const c2rt_path_opts*, const c2rt_temporal_opts*, const c2rt_denoise_variance_opts*,
                                            const c2rt_path_count_opts*, float* out_rgb);
    enum float C2RT_AA_THRESHOLD_REF = 0.1f; /// tooDifferent's default
    int c2rt_render_frame_adaptive_device(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, float threshold,
                                          float* out_rgb_dev, ubyte* needs_aa_dev, void* hip_stream);
    int c2rt_render_frame_adaptive(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, float threshold,
                                   float* out_rgb, ubyte* needs_aa, const(ubyte)* stop_flag);
    /// the same for a batch, with or without a pose per frame: frame i at out + i * W * H * 3 floats, its flags at
    /// needs_aa + i * W * H bytes, the bits of the single-frame adaptive calls; one detection and one refinement
    /// launch for all frames; what a batch and what an adaptive frame refuse, these refuse
    int c2rt_render_frames_adaptive_device(c2rt_ctx*, const c2rt_camera_frame* cams, uint nFrames, const c2rt_render_opts*,
                                           float threshold, float* out_rgb_dev, ubyte* needs_aa_dev, void* hip_stream);
    int c2rt_render_frames_adaptive(c2rt_ctx*, const c2rt_camera_frame* cams, uint nFrames, const c2rt_render_opts*,
                                    float threshold, float* out_rgb, ubyte* needs_aa, const shared(ubyte)* stop_flag);
    int c2rt_render_frames_posed_adaptive_device(c2rt_ctx*, const c2rt_camera_frame* cams, const c2rt_scene_pose* poses,
                                                 uint nFrames, const c2rt_render_opts*, float threshold, float* out_rgb_dev,
                                                 ubyte* needs_aa_dev, void* hip_stream);
    int c2rt_render_frames_posed_adaptive(c2rt_ctx*, const c2rt_camera_frame* cams, const c2rt_scene_pose* poses, uint nFrames,
                                          const c2rt_render_opts*, float threshold, float* out_rgb, ubyte* needs_aa,
                                          const shared(ubyte)* stop_flag);
    /// sample tables: every pixel the average of the caller's n taps (accum = c_0, += c_s in tap order, / cast(float) n),
    /// or, adaptive, taps 1 .. n-1 on the flagged pixels only (n >= 2, offset[0] == (0, 0)); the reference's five taps
    /// give the bits of the C2RT_TAPS_REF5 frame and of c2rt_render_frame_adaptive (include/c2rt.h)
    enum uint C2RT_MAX_SAMPLE_TAPS = 16;
    struct c2rt_tap_table
    {
        uint n;                     /// 1 .. C2RT_MAX_SAMPLE_TAPS
        uint reserved;              /// must be 0
        double[2][C2RT_MAX_SAMPLE_TAPS] offset; /// tap s samples the screen point (x + offset[s][0], y + offset[s][1])
    }
    int c2rt_render_frame_taps_device(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_tap_table*,
                                      float* out_rgb_dev, void* hip_stream);
    int c2rt_render_frame_taps(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_tap_table*,
                               float* out_rgb);
    int c2rt_render_frame_adaptive_taps_device(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*,
                                               const c2rt_tap_table*, float threshold, float* out_rgb_dev,
                                               ubyte* needs_aa_dev, void* hip_stream);
    int c2rt_render_frame_adaptive_taps(c2rt_ctx*, const c2rt_camera_frame*, const c2rt_render_opts*, const c2rt_tap_table*,
                                        float threshold, float* out_rgb, ubyte* needs_aa, const shared(ubyte)* stop_flag);
}

/// Owns the flat tables for one uploaded scene (GC memory; c2rt_upload_scene copies them).
final class GpuScene
{
    c2rt_scene_desc desc;
    private
    {
        int[] geomType, geomChild, texType, shaderType, shaderTexture, lightType, nodeGeom, nodeShader, nodeBump;
        double[] geomParam, texParam, shaderExponent, lightPos, nodeTransform;
        float[] texColor, texScaling, texels, shaderColor, shaderStrength, lightColor, lightPower;
        uint[] texWidth, texHeight;
        ulong[] texOffset;
    }

    private static int indexOf(T)(const T[] all, const Object o)
    {
        foreach (i, e; all) if (e is o) return cast(int) i;
        return -1;
    }

    /// Scene -> c2rt_scene_desc: class references become indices into Scene's arrays.
    this(const Scene scene)
    {
        foreach (g; scene.geometries)
        {
            if (auto p = cast(const Plane) g) { geomType ~= GEOM_PLANE; geomParam ~= [p.y, p.limit, 0, 0]; geomChild ~= [-1, -1]; }
            else if (auto s = cast(const Sphere) g) { geomType ~= GEOM_SPHERE; geomParam ~= [s.center.x, s.center.y, s.center.z, s.R]; geomChild ~= [-1, -1]; }
            else if (auto c = cast(const Cube) g) { geomType ~= GEOM_CUBE; geomParam ~= [c.center.x, c.center.y, c.center.z, c.side]; geomChild ~= [-1, -1]; }
            else if (auto op = cast(const CsgOp) g)
            {
                geomType ~= (cast(const CsgUnion) g) ? GEOM_CSG_UNION : (cast(const CsgInter) g) ? GEOM_CSG_INTER : GEOM_CSG_DIFF;
                geomParam ~= [0.0, 0, 0, 0];
                geomChild ~= [indexOf(scene.geometries, op.left.get), indexOf(scene.geometries, op.right.get)];
            }
        }
        ulong offset = 0;
        foreach (t; scene.textures)
        {
            float[18] col = 0; double[6] par = 0;
            uint w = 0, h = 0; float scaling = 1;
            if (auto c = cast(const Checker) t)
            {
                texType ~= TEX_CHECKER;
                col[0 .. 3] = c.color1.components; col[3 .. 6] = c.color2.components; par[0] = c.size;
            }
            else if (auto p = cast(const Procedure2) t)
            {
                texType ~= TEX_PROCEDURE2;
                foreach (i; 0 .. 3) { col[3*i .. 3*i+3] = p.colorU[i].components; col[9+3*i .. 12+3*i] = p.colorV[i].components;
                                      par[i] = p.freqU[i]; par[3+i] = p.freqV[i]; }
            }
            else if (auto b = cast(const BitmapTexture) t)
            {
                texType ~= TEX_BITMAP; scaling = b.scaling;
                w = cast(uint) b.bmp.width; h = cast(uint) b.bmp.height;
                foreach (px; b.bmp.data.pixels) texels ~= px.components;   // already linear RGB (decompressGamma_sRGB)
            }
            texColor ~= col; texParam ~= par; texScaling ~= scaling; texWidth ~= w; texHeight ~= h; texOffset ~= offset;
            offset += cast(ulong) w * h;
        }
        foreach (s; scene.shaders)
        {
            shaderColor ~= s.color.components;
            if (auto p = cast(const Phong) s)
            { shaderType ~= SHADER_PHONG; shaderTexture ~= indexOf(scene.textures, p.texture.get); shaderExponent ~= p.exponent; shaderStrength ~= p.strength; }
            else
            { auto l = cast(const Lambert) s; shaderType ~= SHADER_LAMBERT; shaderTexture ~= indexOf(scene.textures, l.texture.get); shaderExponent ~= 16; shaderStrength ~= 1; }
        }
        foreach (l; scene.lights)
        {
            auto p = cast(const PointLight) l;
            lightType ~= 0; lightPos ~= [p.pos.x, p.pos.y, p.pos.z]; lightColor ~= l.lightColor.components; lightPower ~= l.lightPower;
        }
        foreach (n; scene.nodes)
        {
            nodeGeom ~= indexOf(scene.geometries, n.geom); nodeShader ~= indexOf(scene.shaders, n.shader);
            nodeBump ~= indexOf(scene.textures, n.bumpmap);
            // gfm mat3d stores c[i][j] row-major in v[0 .. 9]
            nodeTransform ~= n.transform.transform.v[] ~ n.transform.inverseTransform.v[] ~ n.transform.transposedInverse.v[]
                           ~ [n.transform.offset.x, n.transform.offset.y, n.transform.offset.z];
        }
        with (desc)
        {
            n_geoms = cast(uint) geomType.length; geom_type = geomType.ptr; geom_param = geomParam.ptr; geom_child = geomChild.ptr;
            n_textures = cast(uint) texType.length; tex_type = texType.ptr; tex_color = texColor.ptr; tex_param = texParam.ptr;
            tex_scaling = texScaling.ptr; tex_width = texWidth.ptr; tex_height = texHeight.ptr; tex_offset = texOffset.ptr;
            n_texels = offset; texels = this.texels.ptr;
            n_shaders = cast(uint) shaderType.length; shader_type = shaderType.ptr; shader_color = shaderColor.ptr;
            shader_texture = shaderTexture.ptr; shader_exponent = shaderExponent.ptr; shader_strength = shaderStrength.ptr;
            n_lights = cast(uint) lightType.length; light_type = lightType.ptr; light_pos = lightPos.ptr;
            light_color = lightColor.ptr; light_power = lightPower.ptr;
            n_nodes = cast(uint) nodeGeom.length; node_geom = nodeGeom.ptr; node_shader = nodeShader.ptr; node_bump = nodeBump.ptr;
            node_transform = nodeTransform.ptr;
            ambient = scene.settings.ambientLightColor.components;
            max_trace_depth = scene.settings.maxTraceDepth;
            gi_enabled = scene.settings.GIEnabled;
        }
    }
}

/// The six vectors Camera.beginFrame leaves behind (rt/camera.d:77-117) + what getScreenRay reads.
c2rt_camera_frame frameOf(const Camera c)
{
    c2rt_camera_frame f;
    f.pos = c.pos.v; f.up_left = c.upLeft.v; f.up_right = c.upRight.v; f.down_left = c.downLeft.v;
    f.right_dir = c.rightDir.v; f.up_dir = c.upDir.v; f.front_dir = c.frontDir.v;
    f.frame_width = c.frameWidth; f.frame_height = c.frameHeight;
    f.dof = c.dof; f.num_samples = cast(uint) c.numSamples;
    f.focal_plane_dist = c.focalPlaneDist; f.disc_multiplier = c.discMultiplier; f.stereo_separation = c.stereoSeparation;
    return f;
}

/// One per process; created in RTDemo.init, scene uploaded in RTDemo.resetScene after parseSceneFromFile.
final class GpuRenderer
{
    private c2rt_ctx* ctx;
    private GpuScene uploaded;
    private float* pinned;   // the screen buffer currently page-locked through this context

    /// device >= 0: that GPU; device < 0: the current one; allDevices: ONE context over every visible
    /// GPU (c2rt_init_multi(0, null)): frames are dealt to the GPUs in interleaved 8-row strips and every
    /// GPU copies its strips straight into `output.pixels` over its own PCIe link.
    this(int device = -1, bool allDevices = false)
    {
        auto st = allDevices ? c2rt_init_multi(0, null, &ctx) : c2rt_init(device, &ctx);
        enforce(st == C2RT_OK, "no usable GPU");
    }
    ~this()
    {
        if (ctx && pinned) c2rt_unpin_host_buffer(ctx, pinned);
        if (ctx) c2rt_destroy(ctx);
    }

    void upload(const Scene scene)
    {
        uploaded = new GpuScene(scene);
        enforce(c2rt_upload_scene(ctx, &uploaded.desc) == C2RT_OK, c2rt_last_error(ctx).fromStringz);
    }

    /// `screen.alloc` happened (gui/raytracer_demo.d:181-182): let frames stream back at PCIe rate.
    /// The GUI re-allocates `screen` on every resize (gui/raytracer_demo.d:135-143,181-182): the previous
    /// buffer is unpinned first (its pages may already be back with the GC), then the new one is registered.
    void pin(Image!Color screen)
    {
        auto p = cast(float*) screen.pixels.ptr;
        if (pinned && pinned !is p) { c2rt_unpin_host_buffer(ctx, pinned); pinned = null; }
        if (c2rt_pin_host_buffer(ctx, p, screen.pixels.length * Color.sizeof) == C2RT_OK) pinned = p;
    }
    /// Call before the GUI frees or re-allocates the buffer passed to pin().
    void unpin() { if (pinned) { c2rt_unpin_host_buffer(ctx, pinned); pinned = null; } }

    /// Drop-in for `Renderer(scene, output, isRendering, isStopRequested).renderRT()`; call after scene.beginFrame().
    int renderRT(const Scene scene, Image!Color output, shared(bool)* isRendering, const shared(bool)* isStopRequested)
    {
        auto cam = frameOf(scene.camera);
        auto opts = c2rt_render_opts(scene.settings.frameWidth, scene.settings.frameHeight, scene.settings.AAEnabled ? 5 : 1);
        int st = c2rt_render_frame(ctx, &cam, &opts, cast(float*) output.pixels.ptr, cast(const shared(ubyte)*) isStopRequested);
        if (isRendering !is null) (*isRendering).atomicStore(false);   // end(), rt/renderer.d:87-91
        return st;
    }
}

/+ rt/renderer.d, renderSceneAsync — only the lambda body changes:

    scene.beginFrame();
    spawn((shared Scene s, shared Image!Color o, shared(bool)* isWorking, const shared(bool)* isStopping)
        {
            gpuRenderer.renderRT(cast() s, cast() o, isWorking, isStopping);   // was: Renderer(...).renderRT()
        }, cast(shared) scene, cast(shared) output, isRendering, needsRendering);
+/

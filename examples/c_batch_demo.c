/*
 * c_batch_demo.c — many cameras, one scene, one call, from plain C: the demo
 * scene of c_abi_demo.c seen from N cameras on an orbit, rendered by
 * c2rt_render_frames (one mask pre-pass launch and one frame launch for the
 * whole batch) and checked against N c2rt_render_frame calls, bit for bit.
 *
 *   gcc -Iinclude examples/c_batch_demo.c -Lchess2rt_amd -lc2rt -Wl,-rpath,$PWD/chess2rt_amd -lm -o /tmp/c_batch_demo
 *   /tmp/c_batch_demo 160 120 8
 */
#define main c_abi_demo_single_frame_main
#include "c_abi_demo.c" /* demo_scene(), CHECK() */
#undef main

/* the camera turned by `angle` about the vertical axis through (0, *, 100), the middle of the demo scene */
static c2rt_camera_frame orbit(const c2rt_camera_frame *cam, double angle)
{
    c2rt_camera_frame out = *cam;
    const double c = cos(angle), s = sin(angle), px = 0, pz = 100;
    const double *src_p[4] = {cam->pos, cam->up_left, cam->up_right, cam->down_left};
    double *dst_p[4] = {out.pos, out.up_left, out.up_right, out.down_left};
    for (int k = 0; k < 4; ++k) {
        const double x = src_p[k][0] - px, z = src_p[k][2] - pz;
        dst_p[k][0] = px + c * x + s * z;
        dst_p[k][2] = pz - s * x + c * z;
    }
    const double *src_d[3] = {cam->right_dir, cam->up_dir, cam->front_dir};
    double *dst_d[3] = {out.right_dir, out.up_dir, out.front_dir};
    for (int k = 0; k < 3; ++k) {
        dst_d[k][0] = c * src_d[k][0] + s * src_d[k][2];
        dst_d[k][2] = -s * src_d[k][0] + c * src_d[k][2];
    }
    return out;
}

int main(int argc, char **argv)
{
    const uint32_t W = argc > 1 ? (uint32_t)atoi(argv[1]) : 160, H = argc > 2 ? (uint32_t)atoi(argv[2]) : 120;
    uint32_t N = argc > 3 ? (uint32_t)atoi(argv[3]) : 8;
    if (N < 1 || N > C2RT_MAX_BATCH_FRAMES) N = 8;
    c2rt_ctx *ctx = NULL;
    CHECK(c2rt_init(-1, &ctx));

    c2rt_scene_desc sc;
    c2rt_camera_frame cam0;
    demo_scene(&sc, &cam0, W, H);
    CHECK(c2rt_upload_scene(ctx, &sc));

    c2rt_camera_frame *cams = (c2rt_camera_frame *)malloc(N * sizeof *cams);
    for (uint32_t i = 0; i < N; ++i) cams[i] = orbit(&cam0, 2.0 * M_PI * i / N);

    c2rt_render_opts opts;
    memset(&opts, 0, sizeof opts);
    opts.width = W; opts.height = H; opts.taps = C2RT_TAPS_REF5;
    const size_t frame_floats = (size_t)W * H * 3;
    float *batch = (float *)malloc(N * frame_floats * sizeof(float)), *single = (float *)malloc(frame_floats * sizeof(float));
    CHECK(c2rt_render_frames(ctx, cams, N, &opts, batch, NULL));

    int differing = 0;
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(c2rt_render_frame(ctx, &cams[i], &opts, single, NULL));
        const int same = memcmp(single, batch + i * frame_floats, frame_floats * sizeof(float)) == 0;
        double mean = 0;
        for (size_t k = 0; k < frame_floats; ++k) mean += single[k];
        printf("camera %2u: mean %.6f, batch %s the single frame\n", i, mean / (double)frame_floats, same ? "equals" : "DIFFERS FROM");
        differing += !same;
    }
    /* what a batch refuses is refused before anything is enqueued */
    cams[0].dof = 1;
    const int st = c2rt_render_frames(ctx, cams, N, &opts, batch, NULL);
    printf("a depth-of-field camera in the batch -> %d (%s): %s\n", st, c2rt_status_string(st), c2rt_last_error(ctx));
    free(batch);
    free(single);
    free(cams);
    c2rt_destroy(ctx);
    return !(differing == 0 && st == C2RT_ERR_UNSUPPORTED);
}

// rt_guides_host.hpp -- the host half of the guide pass that needs the context (rtgl_guides_frame; rules: rt_guides_plan.hpp, kernel:
// rt_guides.hpp).  Not a header of its own standing: rtgl_amd.hip includes it behind the definitions it uses (rtgl_context, the buffer
// ledger, ensure_wave_buffers, launch_intersect_solo, launch_intersect_split, upload_visit_ids, scene_view) and in front of the entry point.
#pragma once

// options "kernel" and "counters" as the launches of the pass must see them, put back when the pass is in the stream
struct GuidesOptions {
    rtgl_context *ctx; int kernel, counters;
    GuidesOptions(rtgl_context *c, rt_guides_plan::Stage stage) : ctx(c), kernel(c->opt.kernel), counters(c->opt.counters)
    {
        ctx->opt.kernel = rt_guides_plan::stage_kernel(stage, kernel);
        if (!rt_guides_plan::writes(rt_guides_plan::kCounters)) ctx->opt.counters = 0;
    }
    ~GuidesOptions() { ctx->opt.kernel = kernel; ctx->opt.counters = counters; }
};

// ray generation in its lean form, the intersect stage of bounce 0 and guides_kernel<true>
static int launch_guides_mesh(rtgl_context *ctx, rt_guides_plan::Stage stage, const SceneView &sc, const FrameParams &P, const ImageView &im, uint32_t n0, const AovView &aov)
{
    const GuidesOptions options(ctx, stage);
    const uint32_t bounces = rt_guides_plan::wave_bounces();
    RCCHK(ensure_wave_buffers(ctx, n0, bounces, false));
    ctx->wb.batch_rad = nullptr; ctx->wb.batch_px = 0;
    const dim3 grid(rt_guides_plan::blocks(n0));
    // the ray counts and the scan's work counters start at zero, as launch_wavefront starts them
    const uint32_t n_counts = ctx->counts_capacity + 1u <= 256u ? ctx->counts_capacity + 1u : 0u;
    if (!n_counts) HIPCHK(ctx, hipMemsetAsync(ctx->d_counts, 0, counts_bytes(ctx->counts_capacity), ctx->stream));
    uint32_t n_sched = 0u;
    if (stage == rt_guides_plan::kStageSolo && ctx->d_sched && rt_scan_launch::uses_claim_counters(rt_scan_launch::mesh_dist(scan_setup(ctx)))) {
        const size_t words = (size_t)(bounces + 2u) * ctx->wb.sched_stride;
        if (words <= (size_t)grid.x * 256u) n_sched = (uint32_t)words;
        else HIPCHK(ctx, hipMemsetAsync(ctx->d_sched, 0, words * sizeof(uint32_t), ctx->stream));
    }
    hipLaunchKernelGGL(generate_rays_kernel, grid, dim3(256), 0, ctx->stream, P, im, ctx->wb, 0u, n0, (Counters *)nullptr, n_counts, 0u, 0u, n0, n_sched, 1u);
    HIPCHK(ctx, hipGetLastError());
    if (stage == rt_guides_plan::kStageSolo) RCCHK(launch_intersect_solo(ctx, sc, n0, 0u, false, nullptr, nullptr));      // (no decision, no camera: fresh keep bits)
    else RCCHK(launch_intersect_split(ctx, sc, n0, 0u));
    hipLaunchKernelGGL(guides_kernel<true>, grid, dim3(256), 0, ctx->stream, sc, P, im, (const unsigned long long *)ctx->wb.best[0], n0, aov);
    HIPCHK(ctx, hipGetLastError());
    return RTGL_OK;
}

// the pass itself, behind the refusals of rtgl_guides_frame
static int guides_pass(rtgl_context *ctx)
{
    if (ctx->visits_dirty) RCCHK(rebuild_sphere_visits(ctx));
    if (ctx->tris_dirty) RCCHK(rebuild_triangles(ctx));
    RCCHK(upload_visit_ids(ctx));
    const SceneView sc = scene_view(ctx);
    FrameParams P = ctx->params;
    if (!ctx->d_env) P.use_envmap = 0;
    ImageView im{};                                        // (the footprint of render_batch; the pass has no image)
    im.pixels = nullptr; im.width = ctx->width; im.height = ctx->height;
    im.disp_w = ctx->width / 8 * 8; im.disp_h = ctx->height / 8 * 8;
    im.local_rows = ctx->local_rows; im.rank = ctx->rank; im.world = ctx->world; im.strip_rows = ctx->strip_rows;
    int local_disp_rows = 0;
    for (int lr = 0; lr < ctx->local_rows; ++lr) if (rtgl_local_row_to_global(ctx, lr) < im.disp_h) local_disp_rows = lr + 1;
    const uint64_t slots = (uint64_t)im.disp_w * (uint64_t)local_disp_rows;
    if (slots > 0xFFFFFFF0ull) return fail(ctx, RTGL_ERR_INVALID, "rtgl_guides_frame: the image does not fit 32-bit ray slots");
    const uint32_t n0 = (uint32_t)slots;
    const rt_guides_plan::Count count = rt_guides_plan::after_pass({ctx->aov_n, ctx->aov_restart});
    AovView aov{};
    aov.albedo = ctx->d_aov[0]; aov.normal = ctx->d_aov[1]; aov.position = ctx->d_aov[2]; aov.ids = ctx->d_aov_ids;
    aov.visit_mesh = ctx->d_visit_mesh; aov.visit_tri = ctx->d_visit_tri; aov.n = count.n;
    if (rt_guides_plan::enqueues(n0)) {
        const rt_guides_plan::Stage stage = rt_guides_plan::stage(ctx->opt.kernel, sc.n_tri_visits);
        HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        if (rt_guides_plan::generates_rays(stage)) RCCHK(launch_guides_mesh(ctx, stage, sc, P, im, n0, aov));
        else {
            hipLaunchKernelGGL(guides_kernel<false>, dim3(rt_guides_plan::blocks(n0)), dim3(256), 0, ctx->stream, sc, P, im, (const unsigned long long *)nullptr, n0, aov);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        ctx->last_batch_frames = 1; ctx->timed = true;     // (rtgl_last_frame_ms covers the pass)
    }
    ctx->aov_n = count.n; ctx->aov_restart = count.restart;
    return RTGL_OK;
}

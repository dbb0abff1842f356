// rtgl_amd.hip -- HIP kernels + C ABI (include/rtgl_amd.h) of the MI355X-native path tracer.
// gfx950 only.  Build: see raytracer.glsl_amd/csrc/Makefile (hipcc --offload-arch=gfx950
// -ffp-contract=off).  There is no CPU fallback: without a HIP device every entry point fails.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <mutex>
#include <thread>
#include <type_traits>
#include <condition_variable>
#include <memory>

#include "../../include/rtgl_amd.h"
#include "rt_device.hpp"
#include "rt_wavefront.hpp"
#include "rt_mfma.hpp"
#include "rt_scan.hpp"
#include "rt_denoise.hpp"
#include "rt_denoise_plan.hpp"
#include "rt_temporal.hpp"
#include "rt_temporal_clip.hpp"
#include "rt_temporal_plan.hpp"
#include "rt_tonemap.hpp"
#include "rt_tonemap_plan.hpp"
#include "rt_error.hpp"
#include "rt_error_plan.hpp"
#include "rt_adaptive.hpp"
#include "rt_adaptive_plan.hpp"
#include "rt_robust.hpp"
#include "rt_robust_plan.hpp"
#include "rt_spread.hpp"
#include "rt_spread_plan.hpp"
#include "rt_robust_tiles.hpp"
#include "rt_robust_tiles_plan.hpp"
#include "rt_bucket_guide.hpp"
#include "rt_bucket_guide_plan.hpp"
#include "rt_guides.hpp"
#include "rt_guides_plan.hpp"
#include "rt_node_walk.hpp"
#include "rt_mesh_visits.hpp"
#include "rt_buffers.hpp"
#include "rt_scan_launch.hpp"
#include "rt_shade_launch.hpp"
#include "rt_camera_keep.hpp"
#include "rt_options.hpp"

#pragma clang fp contract(off)

using namespace rt;

// =================================================================================================
// Kernels
// =================================================================================================

// ---- upload-time preparation -------------------------------------------------------------------
// One thread per triangle visit.  visit_tri[k] = triangle index tested k-th by the reference's
// mesh loops (find_closest_mesh :336-341: meshes in order, each over [start, start + size) with the sum taken in 32 bits as the
// shader takes it -- a sum that wraps ends the loop early or empties it -- and without the indices past the vertex buffer, whose
// all-zero triangles no ray can hit: rt_mesh_visits.hpp).
__global__ void __launch_bounds__(256) prepare_triangles_kernel(const float4 *__restrict__ vertices,
                                                                const uint32_t *__restrict__ visit_tri, uint32_t n_visits,
                                                                TriEdges *__restrict__ edges, TriPlane *__restrict__ planes)
{
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_visits) return;
    uint32_t tri = visit_tri[k];
    float4 a = vertices[3 * (size_t)tri + 0], b = vertices[3 * (size_t)tri + 1], c = vertices[3 * (size_t)tri + 2];
    f3 v0 = mk(a.x, a.y, a.z), v1 = mk(b.x, b.y, b.z), v2 = mk(c.x, c.y, c.z);
    f3 e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2;                                   // :230,233,236
    f3 m0 = cross3(v1, v0), m1 = cross3(v2, v1), m2 = cross3(v0, v2);              // :231,234,237
    f3 n = normalize3(cross3(v1 - v0, v2 - v0));                                   // :239
    TriEdges E;
    E.e0x = e0.x; E.e0y = e0.y; E.e0z = e0.z; E.e1x = e1.x; E.e1y = e1.y; E.e1z = e1.z; E.e2x = e2.x; E.e2y = e2.y; E.e2z = e2.z;
    E.m0x = m0.x; E.m0y = m0.y; E.m0z = m0.z; E.m1x = m1.x; E.m1y = m1.y; E.m1z = m1.z; E.m2x = m2.x; E.m2y = m2.y; E.m2z = m2.z;
    float be = fmaxf(fmaxf(dot3(e0, e0), dot3(e1, e1)), dot3(e2, e2));
    float bm = fmaxf(fmaxf(dot3(m0, m0), dot3(m1, m1)), dot3(m2, m2));
    E.bound_e = __builtin_sqrtf(be) * 1.0001f;
    E.bound_m = __builtin_sqrtf(bm) * 1.0001f;
    edges[k] = E;
    TriPlane P;
    P.nx = n.x; P.ny = n.y; P.nz = n.z; P.v0x = v0.x; P.v0y = v0.y; P.v0z = v0.z;
    float w = a.w;                                                                 // int(vertices[3v].w) :353
    P.material = (w > -2147483648.0f && w < 2147483648.0f) ? (int32_t)w : -1;
    P.pad = 0;
    planes[k] = P;
}

// ---- variant 0: megakernel, one lane per pixel ----------------------------------------------------
// Triangle records are wave-uniform, so the compiler fetches them with scalar loads (SGPR operands
// feed the fma chain directly); no LDS traffic.  Baseline variant, kept as the A/B reference for the
// tiled / wavefront kernels.
// kAov: option "aov" is on -- the camera ray's hit (bounce 0 of sample 0) also goes to the first-hit planes (rt_wavefront.hpp, aov_write)
template <bool kCount, bool kAov>
__global__ void __launch_bounds__(256) pathtrace_mega_kernel(SceneView sc, FrameParams P, ImageView im, uint4 *rng_out, Counters *counters, AovView aov)
{
    // 8x8 pixel block per wave (matches the reference work-group shape :38), 4 waves side by side
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = (blockIdx.x * 4 + wave) * 8 + (lane & 7);
    const int lrow = blockIdx.y * 8 + (lane >> 3);
    if (px >= im.disp_w || lrow >= im.local_rows) return;
    const int py = local_to_global_row(im, lrow);
    if (py >= im.disp_h) return;

    Rng rng; rng.x = (uint32_t)px; rng.y = (uint32_t)py; rng.z = (uint32_t)P.random;       // init_rand :135-138
    rng.w = (uint32_t)px + (uint32_t)py + (uint32_t)P.random;
    float4 *pix = im.pixels + (size_t)lrow * im.width + px;
    f3 prev = mk(0.0f, 0.0f, 0.0f);
    if (!P.reset_flag) { float4 q = *pix; prev = mk(q.x, q.y, q.z); }                       // :542-548
    f3 origin, dir;
    camera_ray(P, px, py, im.width, im.height, rng, origin, dir);

    unsigned long long c_seg = 0, c_tests = 0, c_cand = 0, c_env = 0;
    f3 color = mk(0.0f, 0.0f, 0.0f);
    for (uint32_t s = 0; s < P.samples; ++s) {                                              // :556-559
        f3 o = origin, d = dir;
        f3 radiance = mk(0.0f, 0.0f, 0.0f), thr = mk(1.0f, 1.0f, 1.0f);
        for (uint32_t bounce = 0; bounce < P.max_bounce; ++bounce) {                        // :425
            if (kCount) c_seg++;
            Hit h1; h1.t = kInf; h1.material = 0; h1.point = h1.normal = mk(0.0f, 0.0f, 0.0f);
            uint32_t sphere_id = kNoSphere;
            bool hit_sphere = kAov ? sphere_pass_id(sc, o, d, h1, sphere_id) : sphere_pass(sc, o, d, h1);   // :433
            // find_closest_mesh (:331-361)
            TriRay tr = make_tri_ray(o, d);
            float best_t = kInf; uint32_t best_v = 0xFFFFFFFFu;
            for (uint32_t v = 0; v < sc.n_tri_visits; ++v) {
                const TriEdges &T = sc.tri_edges[v];
                if (tri_filter(T, tr)) {
                    if (kCount) c_cand++;
                    float t = tri_exact(T, sc.tri_planes[v], tr);
                    if (kEps < t && t < best_t) { best_t = t; best_v = v; }
                }
            }
            if (kCount) c_tests += sc.n_tri_visits;
            bool hit_mesh = best_v != 0xFFFFFFFFu;
            if (!hit_sphere && !hit_mesh) {                                                 // :441-445
                f3 bg;
                if (P.use_envmap) { bg = env_lookup(sc, d); if (kCount) c_env++; }
                else bg = mk(P.background[0], P.background[1], P.background[2]);
                if (kAov && s == 0u && bounce == 0u) aov_write(sc, aov, (uint32_t)(lrow * im.width + px), kAovMiss, h1, 0u, bg);
                radiance = radiance + bg * thr;
                break;
            }
            Hit h = h1;
            if (!(h1.t < best_t)) {                                                         // :447
                const TriPlane &pl = sc.tri_planes[best_v];
                h.t = best_t; h.point = o + d * best_t; h.normal = mk(pl.nx, pl.ny, pl.nz); h.material = pl.material;
            }
            if (kAov && s == 0u && bounce == 0u)
                aov_write(sc, aov, (uint32_t)(lrow * im.width + px), !(h1.t < best_t) ? kAovTriangle : kAovSphere, h, !(h1.t < best_t) ? best_v : sphere_id, mk(0.0f, 0.0f, 0.0f));
            if (!shade_hit(sc, h, rng, o, d, thr, radiance)) break;
        }
        color = color + radiance;
    }
    if (kAov && P.max_bounce == 0u) {                    // no ray was traced: a miss that received nothing
        Hit none; none.t = kInf; none.material = 0; none.point = none.normal = mk(0.0f, 0.0f, 0.0f);
        aov_write(sc, aov, (uint32_t)(lrow * im.width + px), kAovMiss, none, 0u, mk(0.0f, 0.0f, 0.0f));
    }
    { const float4 v = accumulate_pixel(P, color, prev); store_through(pix, v.x, v.y, v.z, v.w); }      // (rt_wavefront.hpp: read by the next frame's kernel, from whichever XCD)
    if (rng_out) rng_out[(size_t)lrow * im.width + px] = make_uint4(rng.x, rng.y, rng.z, rng.w);
    if (kCount) {
        atomicAdd(&counters->paths, (unsigned long long)P.samples);
        atomicAdd(&counters->segments, c_seg);
        atomicAdd(&counters->tri_tests, c_tests);
        atomicAdd(&counters->candidates, c_cand);
        atomicAdd(&counters->env_lookups, c_env);
    }
}

// ---- 8-bit readback (glGetTexImage GL_UNSIGNED_BYTE, src/renderer.cpp:223) -----------------------
__global__ void __launch_bounds__(256) image_to_u8_kernel(const float4 *__restrict__ src, uchar4 *__restrict__ dst, int width, int rows, int flip)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * rows) return;
    int y = i / width, x = i - y * width;
    float4 p = src[i];
    auto q = [](float v) -> unsigned char {
        v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);      // NaN -> 0 like a clamp-to-[0,1] conversion
        if (!(v == v)) v = 0.0f;
        return (unsigned char)__builtin_rintf(v * 255.0f);
    };
    int oy = flip ? rows - 1 - y : y;
    dst[(size_t)oy * width + x] = make_uchar4(q(p.x), q(p.y), q(p.z), q(p.w));
}

// =================================================================================================
// Host side: context + C ABI
// =================================================================================================

static thread_local std::string g_create_error;

// rtgl_create_multi: one submit thread per part.  A frame is ~27 launches = ~150 us of host time per device (measured,
// tools/diagnostics/host_enqueue.py) while a rank of 8 renders its strips of the 1080p benchmark frame in 0.68 ms: ONE thread submitting
// to 8 devices one after the other (1.2 ms) would be the limiter, 8 threads side by side are not.
struct PartWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    enum { kIdle, kJob, kDone, kQuit } state = kIdle;
    int rc = 0;
    rtgl_context *part = nullptr;
};

// the ledger's allocator and deallocator: the only two calls of their kind in this file
static int device_alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
static int device_free(void *p) { return (int)hipFree(p); }

// What a session of masked tiles owns, whichever kind it is (rt_adaptive_plan.hpp): the sample buffer a masked frame traces into, the tile
// records, the counts (n per tile, then m per tile) and the two lists a frame reads (the active blocks, then the active tiles).
// active: a session is open; the mask and the lists as they are on the device
struct TileSession {
    float4 *d_samples = nullptr; uint4 *d_records = nullptr; uint32_t *d_counts = nullptr, *d_lists = nullptr;
    bool active = false;
    std::vector<uint8_t> mask; std::vector<uint32_t> blocks, tiles;
};

struct rtgl_context {
    int device = 0;
    int width = 0, height = 0;
    int rank = 0, world = 1, strip_rows = 8, local_rows = 0;
    hipStream_t own_stream = nullptr, stream = nullptr; bool own_stream_shared = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    // kernel_timing: events since the last rtgl_timing_reset.  Per frame: [frame begin, (launch begin, launch end)*, frame end]
    std::vector<hipEvent_t> kev;
    uint32_t kev_used = 0;
    std::vector<uint32_t> kev_frame_start;   // index into kev of each recorded frame's first event
    std::string error;

    // raw scene copies (host) used to rebuild derived buffers
    std::vector<uint8_t> h_meshes, h_nodes, h_vertices;
    uint32_t n_meshes = 0, n_nodes = 0, n_vec4 = 0;

    // device buffers: every one of them is allocated, grown and freed through `buffers` (rt_buffers.hpp), keyed by its pointer field here
    rt_buffers::Ledger buffers{device_alloc, device_free};
    SphereRec *d_spheres = nullptr; uint32_t n_spheres = 0;
    MaterialRec *d_materials = nullptr; uint32_t n_materials = 0;
    float4 *d_vertices = nullptr;
    uint32_t *d_sphere_visits = nullptr; uint32_t n_sphere_visits = 0;
    TriEdges *d_edges = nullptr; TriPlane *d_planes = nullptr; uint32_t n_tri_visits = 0;
    TriEdges *d_edges_s = nullptr; TriPlane *d_planes_s = nullptr;          // ... in the storage order of the matrix-core scan (narrow phase)
    uint8_t *d_env = nullptr; int env_w = 0, env_h = 0, env_c = 0, env_faces = 0;
    float4 *d_image_own = nullptr, *d_image = nullptr;
    uint4 *d_rng = nullptr;
    Counters *d_counters = nullptr;
    uchar4 *d_u8 = nullptr;

    // bounce-wavefront pipeline buffers
    float2 *d_group_bounds = nullptr;
    MfGroup *d_mf_groups = nullptr; MfCull *d_mf_cull = nullptr; MfCull *d_mf_cull_node = nullptr; uint32_t cull_node_shift = 0; uint4 *d_mf_A = nullptr; uint32_t *d_mf_order = nullptr; uint32_t n_mf_groups = 0, mf_group_quads = 32; uint32_t *d_dbg_log = nullptr;   // bf16 matrix-core broad phase
    void *d_wave = nullptr; size_t wave_capacity = 0; bool wave_multi = false;   // queues (+ per-pixel state when u_samples > 1)
    uint32_t *d_counts = nullptr; uint32_t counts_capacity = 0;
    uint32_t *h_counts = nullptr;            // pinned: ray counts per bounce of the most recent finished frame
    hipEvent_t counts_ev = nullptr; bool counts_pending = false, counts_valid = false;
    bool timing_this_frame = false; uint32_t timing_frame_counter = 0;
    int kernel_in_use = -1;                  // variant the last frame actually ran
    int n_cus = 256;
    // kernel 4 candidate buffer: one region per wave of a scan launch.  Sized from what the scene needs, not from the image: it starts
    // at one record per ray and grows to 1.25 x the fullest region any finished frame reported (records that do not fit are tested
    // in place by the scan, so every size is correct; a too small one is only slower)
    uint2 *d_items = nullptr; size_t items_capacity = 0;          // packet culling: per chunk of a culled scan launch its work items + one count per chunk
    uint32_t *d_sched = nullptr; size_t sched_capacity = 0;       // kernel 4: next unclaimed item per (bounce, chunk)
    uint32_t *d_keep = nullptr; size_t keep_capacity = 0;         // packet culling: (granules of 128 rays) x (tiles / 32) words
    // the camera-ray bounce's keep bits, kept across frames while camera, image and scene stand still (a progressive render's normal state):
    // the camera rays of two frames differ by the depth-of-field jitter only, so bits certified for one frame's rays with the packet bounds
    // widened by that jitter hold for all of them and packet_cull_kernel is skipped on bounce 0 (a third of its work)
    uint32_t *d_keep0 = nullptr; size_t keep0_capacity = 0; bool keep0_valid = false; rt_camera_keep::Camera keep0_camera{}; uint32_t keep0_n0 = 0, keep0_words = 0; uint64_t keep0_scene = 0;
    uint32_t camera_lean_frames = 0;                        // frames of this context that took the lean camera bounce (option "camera_lean")
    uint32_t shade_pass_launches = 0;                       // launches of this context that took the one-pass shade_kernel (option "shade_pass")
    uint64_t scene_version = 0;
    void *d_plan = nullptr; size_t plan_capacity = 0;             // planned work distribution of culled scan launches: cost prefix sums per chunk
    void *d_stage = nullptr; size_t stage_capacity = 0;           // ray binning: the staging queue + (key, rank) and the source slot per slot
    uint32_t *d_sort_hist = nullptr; uint32_t sort_bits_alloc = 0;      // two sets of bin counters, used in turns
    bool bin_refusal_said = false;                                     // a refused RTGL_AMD_SORT_OB / _DB pair was reported on stderr
    int sort_set = 0; uint32_t sort_set_bits = 0; bool sort_sets_clean = false;      // the set the next binned bounce counts in; false: zero both first (fresh, or a frame was abandoned half way)
    float mesh_lo[3] = {0.0f, 0.0f, 0.0f}, mesh_hi[3] = {0.0f, 0.0f, 0.0f}, mesh_ext = 0.0f;       // box of the triangles' finite vertices (origin cells of the bin key)
    uint2 *d_cand = nullptr; uint32_t cand_regions = 0, cand_region_pairs = 0, cand_region_target = 0; bool cand_fixed = false;
    bool solo_attr_set = false;              // hipFuncAttributeMaxDynamicSharedMemorySize is per device: raised once per context (= per device binding)
    bool group_explicit = false;             // "mf_group_quads" was set through rtgl_set_option
    bool kernel_explicit = false;            // "kernel" was set through rtgl_set_option or RTGL_AMD_KERNEL
    uint32_t counts_n0 = 0, counts_len = 0;
    std::vector<uint32_t> est_counts;        // grid-size estimates for the next frame
    WaveBuffers wb{};

    // single-process multi-device mode (rtgl_create_multi): this context is the assembler -- it owns the full image on devices[0] --
    // and `parts` are the per-device tiled contexts that render the strips; every entry point fans out to them
    std::vector<rtgl_context *> parts;
    std::vector<hipEvent_t> part_done;
    hipEvent_t gather_done = nullptr;                     // recorded behind the gather's copies; every part waits for it before its next frame
    std::vector<std::unique_ptr<PartWorker>> workers;     // one per part when there is more than one (RTGL_AMD_MULTI_THREADS=0: none, the caller's thread submits)
    bool gathered = false, peer_copy = true;

    // frame batching (option "frame_batch" = B > 1): rtgl_render_frame only records the frame's uniforms until B frames are waiting (or
    // anything else is asked of the context); the B frames then travel through one set of launches (render_batch)
    std::vector<FrameParams> pending;
    float4 *d_batch_rad = nullptr; size_t batch_capacity = 0;
    uint32_t last_batch_frames = 1;
    bool tris_dirty = false, visits_dirty = false;
    // first-hit planes (option "aov"): one buffer of local_rows x width 16-byte records per enabled plane (albedo, normal, position, ids);
    // aov_n frames in their running mean, restarted by the next frame when aov_restart is set
    float4 *d_aov[3] = {nullptr, nullptr, nullptr}; uint4 *d_aov_ids = nullptr;
    uint32_t aov_n = 0; bool aov_restart = true;
    // ... and, for the ids plane only, per triangle visit its mesh and its triangle (uploaded while that plane is enabled)
    std::vector<uint32_t> h_visit_mesh, h_visit_tri;
    uint32_t *d_visit_mesh = nullptr, *d_visit_tri = nullptr; bool visit_ids_dirty = true;
    uint32_t *d_visit_scratch = nullptr;     // rebuild_triangles: the visit list while the upload-time kernels run; freed at its end (after a failed rebuild: by the next one)
    // rtgl_denoise: two RGBA32F buffers the passes alternate between and the buffer the last pass writes, each local_rows x width records,
    // allocated by the first call that needs them; has_denoised: a call has succeeded, so the read-out calls have something to return
    float4 *d_dn_scratch[2] = {nullptr, nullptr}, *d_denoised = nullptr; bool has_denoised = false;
    // rtgl_denoise_guided: shares the three buffers above; its variance buffer {mu, v0, var, s0}, local_rows x width records
    float4 *d_dn_variance = nullptr; uint32_t *d_dn_near = nullptr; bool has_dn_variance = false;      // (d_dn_near: one word per pixel)
    // rtgl_temporal_accumulate: two history buffers {rgb, n} and two copies each of the position and the normal plane, taking turns;
    // tm_cur: the set the latest call wrote.  has_temporal: a call has succeeded (read-out, "denoise_source"); tm_valid: the next call
    // may reproject from set tm_cur (false after rtgl_temporal_reset); tm_has_normal: that set holds a copy of the normal plane
    float4 *d_tm_hist[2] = {nullptr, nullptr}, *d_tm_normal[2] = {nullptr, nullptr}, *d_tm_position[2] = {nullptr, nullptr};
    int tm_cur = 0; bool has_temporal = false, tm_valid = false, tm_has_normal = false;
    TemporalCamera tm_camera{};
    // option "temporal_moments": two buffers of records {m1, m2, v, n} that take turns with the history's (set tm_cur), allocated by the
    // first call that needs them; tm_moments: the mode (1, 2) whose records the latest successful call stored in set tm_cur, 0: none
    float4 *d_tm_moments[2] = {nullptr, nullptr}; int tm_moments = 0;
    // rtgl_tonemap: the RGBA8 display buffer and the state the kernels share (two histogram sets that take turns and the exposure,
    // rt_tonemap.hpp), allocated by the first call.  has_display: a call has succeeded; tone: the turn of the two sets
    // (rt_tonemap_plan.hpp); tone_auto: the latest call solved its exposure on the device, otherwise it used tone_exposure
    uchar4 *d_display = nullptr; uint32_t *d_tone_state = nullptr;
    bool has_display = false, tone_auto = false; rt_tonemap_plan::Sets tone; float tone_exposure = 1.0f;
    // rtgl_error_estimate (rt_error.hpp): the luminance snapshot, the tile records and the summary, allocated by the first call.  err:
    // what the host knows of the accumulation and of the snapshot (rt_error_plan.hpp); every event that drops the snapshot (header,
    // "error estimate") goes through rt_error_plan::drop
    float *d_err_snapshot = nullptr; uint4 *d_err_tiles = nullptr; uint32_t *d_err_summary = nullptr;
    rt_error_plan::Snapshot err; bool has_error = false;
    // adaptive sampling (rt_adaptive.hpp, rt_adaptive_plan.hpp), all allocated by the first rtgl_adaptive_begin: the session's masked tiles
    // and the snapshot plane.  has_adaptive: a begin has succeeded, so the tile records can be read
    TileSession ad; float *d_ad_snapshot = nullptr;
    bool has_adaptive = false; rtgl_adaptive_params ad_params{};
    // robust accumulation (rt_robust.hpp, rt_robust_plan.hpp), allocated by rtgl_robust_begin and freed by rtgl_robust_end: the rb_K bucket
    // planes (bucket-major) and the output plane.  rb_active: a session is open; rb_N: the frames folded; rb_resolved: the output plane holds a resolve
    float4 *d_rb_buckets = nullptr, *d_rb_out = nullptr;
    uint32_t rb_K = 0, rb_N = 0; bool rb_active = false, rb_resolved = false;
    // rtgl_robust_error_estimate (rt_spread.hpp, rt_spread_plan.hpp): the tile records and the summary of the session, allocated by its
    // first estimate and freed by rtgl_robust_end.  has_rb_error: an estimate of THIS session has succeeded
    uint4 *d_rbe_tiles = nullptr; uint32_t *d_rbe_summary = nullptr; bool has_rb_error = false;
    // a robust adaptive session (rt_robust_tiles.hpp, rt_robust_tiles_plan.hpp), allocated by rtgl_robust_adaptive_begin and freed by
    // rtgl_robust_adaptive_end: the session's masked tiles, the ra_K bucket planes (bucket-major) and the output plane.
    // ra_resolved: the output plane holds a resolve
    TileSession ra; float4 *d_ra_buckets = nullptr, *d_ra_out = nullptr;
    uint32_t ra_K = 0; bool ra_resolved = false; rt_robust_tiles_plan::Params ra_params{};
    FrameParams params{};
    bool have_params = false;
    rt_options::Options opt;                 // every integer option, with its default (rt_options.hpp)
};
static_assert(rt_options::kKernelMega == RTGL_KERNEL_MEGA && rt_options::kKernelRemoved3 == RTGL_KERNEL_REMOVED_3 && rt_options::kKernelSolo == RTGL_KERNEL_WAVEFRONT_MFMA_SOLO && rt_options::kAovAll == RTGL_AOV_ALL && rt_options::kScalar == kScalar && rt_options::kLds == kLds, "rt_options.hpp");
static_assert(rt_options::kBoundGroup == kBoundGroup && (uint32_t)rt_options::kMaxChunk == kMaxChunk && (uint32_t)rt_options::kMfMaxChunkQuads == kMfMaxChunkQuads && (uint32_t)rt_options::kMfMaxGroupQuads == kMfMaxGroupQuads && (uint32_t)rt_options::kBatchMax == kBatchMax, "rt_options.hpp");

static int fail(rtgl_context *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->error = msg; else g_create_error = msg;
    return code;
}
#define HIPCHK(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return fail(ctx, RTGL_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

#define RCCHK(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// typed fronts of the context's ledger; a failure is the usual RTGL_ERR_DEVICE
static int buf_rc(rtgl_context *ctx, const char *what, int e) { return e ? fail(ctx, RTGL_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString((hipError_t)e)) : RTGL_OK; }
template <typename T> static int buf_alloc(rtgl_context *ctx, T *&p, size_t bytes) { return buf_rc(ctx, "device allocation", ctx->buffers.allocate((void **)&p, bytes)); }
template <typename T> static int buf_ensure(rtgl_context *ctx, T *&p, size_t bytes) { return buf_rc(ctx, "device allocation", ctx->buffers.ensure((void **)&p, bytes)); }
template <typename T, typename C> static int buf_grow(rtgl_context *ctx, T *&p, C &capacity, size_t need, size_t bytes) { return buf_rc(ctx, "device allocation", ctx->buffers.grow((void **)&p, capacity, (C)need, bytes)); }
template <typename... T> static int buf_release(rtgl_context *ctx, T *&...p)      // stops at the first free that fails
{
    int e = 0;
    ((e = e ? e : ctx->buffers.release((void **)&p)), ...);
    return buf_rc(ctx, "device free", e);
}

static size_t local_px(const rtgl_context *ctx) { return (size_t)std::max(ctx->local_rows, 1) * ctx->width; }      // (a tile without rows still owns one)

// the context's rows of a buffer of `px_bytes` bytes per pixel, on the host when this returns
static int read_rows(rtgl_context *ctx, void *dst, const void *src, size_t px_bytes)
{
    HIPCHK(ctx, hipMemcpyAsync(dst, src, (size_t)ctx->local_rows * ctx->width * px_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RTGL_OK;
}

// The two getters of a plane that one call writes.  `ready`: that call has succeeded; otherwise the message is `who` + `why`.  `what`: the
// whole message for a NULL `dst` (some entry points say it with their name, some without)
static int read_plane(rtgl_context *ctx, void *dst, const char *what, bool ready, const void *src, size_t px_bytes, const char *who, const char *why)
{
    if (!dst) return fail(ctx, RTGL_ERR_INVALID, what);
    if (!ready) return fail(ctx, RTGL_ERR_STATE, std::string(who) + why);
    return read_rows(ctx, dst, src, px_bytes);
}
static void *device_plane(rtgl_context *ctx, bool ready, const void *ptr, const char *who, const char *why)
{
    if (!ready) { ctx->error = std::string(who) + why; return nullptr; }
    return (void *)ptr;
}

template <typename T>
static int realloc_upload(rtgl_context *ctx, T *&dptr, const void *src, size_t bytes)
{
    if (bytes == 0) return buf_release(ctx, dptr);
    RCCHK(buf_alloc(ctx, dptr, bytes));
    if (src) HIPCHK(ctx, hipMemcpyAsync(dptr, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // uploads are synchronous like glBufferData
    return RTGL_OK;
}

static int local_rows_for(int height, int rank, int world, int strip_rows)
{
    int n_strips = (height + strip_rows - 1) / strip_rows, rows = 0;
    for (int s = rank; s < n_strips; s += world) rows += std::min(strip_rows, height - s * strip_rows);
    return rows;
}

// Every context of a process on one device submits to ONE stream (unless the caller binds its own with rtgl_set_stream): the kernels
// of different contexts then never run beside each other.  Several path-tracing pipelines running CONCURRENTLY on a device have
// produced wrong frames (16 rays of a launch scanning stale data; DESIGN.md 5.2 -- rare with the shipped kernels, cause not
// established); a single pipeline at a time never has.  RTGL_AMD_PRIVATE_STREAMS=1 restores one stream per context (diagnostics:
// tools/diagnostics/flaky_tiled.py).
static std::mutex g_stream_mutex;
static std::map<int, std::pair<hipStream_t, int>> g_device_streams;
static hipError_t acquire_device_stream(int device, hipStream_t *out, bool *shared)
{
    const char *priv = getenv("RTGL_AMD_PRIVATE_STREAMS");
    if (priv && atoi(priv) != 0) { *shared = false; return hipStreamCreateWithFlags(out, hipStreamNonBlocking); }
    std::lock_guard<std::mutex> lock(g_stream_mutex);
    auto it = g_device_streams.find(device);
    if (it == g_device_streams.end()) {
        hipStream_t st = nullptr;
        const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
        it = g_device_streams.emplace(device, std::make_pair(st, 0)).first;
    }
    it->second.second++;
    *out = it->second.first; *shared = true;
    return hipSuccess;
}
// Which stream every live context of this process submits to, per device: rtgl_set_stream refuses a binding that would put two
// path-tracing pipelines on DIFFERENT streams of one device (they could then run concurrently: DESIGN.md 5.2) unless the caller takes
// that over explicitly (RTGL_AMD_ALLOW_CONCURRENT_PIPELINES=1; RTGL_AMD_PRIVATE_STREAMS=1 implies it).
static std::map<const rtgl_context *, std::pair<int, hipStream_t>> g_ctx_streams;
static void register_ctx_stream(const rtgl_context *ctx, int device, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(g_stream_mutex);
    g_ctx_streams[ctx] = std::make_pair(device, st);
}
static void unregister_ctx_stream(const rtgl_context *ctx)
{
    std::lock_guard<std::mutex> lock(g_stream_mutex);
    g_ctx_streams.erase(ctx);
}
static bool other_stream_in_use(const rtgl_context *ctx, int device, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(g_stream_mutex);
    for (const auto &kv : g_ctx_streams) if (kv.first != ctx && kv.second.first == device && kv.second.second != st) return true;
    return false;
}
static bool concurrent_pipelines_allowed()
{
    const char *a = getenv("RTGL_AMD_ALLOW_CONCURRENT_PIPELINES"), *p = getenv("RTGL_AMD_PRIVATE_STREAMS");
    return (a && atoi(a) != 0) || (p && atoi(p) != 0);
}

static void release_device_stream(int device, hipStream_t st, bool shared)
{
    if (!shared) { (void)hipStreamDestroy(st); return; }
    std::lock_guard<std::mutex> lock(g_stream_mutex);
    auto it = g_device_streams.find(device);
    if (it != g_device_streams.end() && --it->second.second == 0) { (void)hipStreamDestroy(it->second.first); g_device_streams.erase(it); }
}

extern "C" int rtgl_create_tiled(rtgl_context **out, int width, int height, int device, int rank, int world, int strip_rows)
{
    if (!out) return fail(nullptr, RTGL_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (width <= 0 || height <= 0 || world < 1 || rank < 0 || rank >= world || strip_rows <= 0 || (strip_rows % 8) != 0)
        return fail(nullptr, RTGL_ERR_INVALID, "rtgl_create: bad size / tiling arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, RTGL_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(nullptr, RTGL_ERR_INVALID, "device ordinal out of range");
    rtgl_context *ctx = new rtgl_context();
    ctx->device = device; ctx->width = width; ctx->height = height;
    ctx->rank = rank; ctx->world = world; ctx->strip_rows = strip_rows;
    ctx->local_rows = local_rows_for(height, rank, world, strip_rows);
    auto bail = [&](int code) { g_create_error = ctx->error; rtgl_destroy(ctx); return code; };
#define CCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    ctx->error = std::string(#expr) + ": " + hipGetErrorString(e_); return bail(RTGL_ERR_DEVICE); } } while (0)
    CCHK(hipSetDevice(device));
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ctx->n_cus = prop.multiProcessorCount; }
    CCHK(acquire_device_stream(device, &ctx->own_stream, &ctx->own_stream_shared));
    ctx->stream = ctx->own_stream;
    register_ctx_stream(ctx, device, ctx->stream);
    CCHK(hipEventCreate(&ctx->ev0));
    CCHK(hipEventCreate(&ctx->ev1));
    size_t img_bytes = local_px(ctx) * sizeof(float4);
    if (buf_alloc(ctx, ctx->d_image_own, img_bytes)) return bail(RTGL_ERR_DEVICE);
    CCHK(hipMemsetAsync(ctx->d_image_own, 0, img_bytes, ctx->stream));
    ctx->d_image = ctx->d_image_own;
    if (buf_alloc(ctx, ctx->d_counters, 64)) return bail(RTGL_ERR_DEVICE);
    CCHK(hipMemsetAsync(ctx->d_counters, 0, 64, ctx->stream));
    CCHK(hipStreamSynchronize(ctx->stream));
#undef CCHK
    // the environment's spellings of the options (rt_options.hpp) change this context's defaults; rtgl_set_option still wins.  RTGL_AMD_KERNEL=0, 1, 2
    // or 4: the operational override of the default scan without touching the caller
    const uint32_t from_env = rt_options::read_environment(ctx->opt, [](const char *name) -> const char * { return getenv(name); });
    if (from_env & rt_options::row_bit(&rt_options::Options::kernel)) ctx->kernel_explicit = true;
    *out = ctx;
    return RTGL_OK;
}

static int flush_pending(rtgl_context *ctx);
extern "C" int rtgl_create(rtgl_context **out, int width, int height, int device)
{
    return rtgl_create_tiled(out, width, height, device, 0, 1, 8);
}

extern "C" void rtgl_destroy(rtgl_context *ctx)
{
    if (!ctx) return;
    // frames a batching context still holds back are submitted, not dropped (a caller that only ever called rtgl_render_frame and then
    // reads a bound device image after destroying the context would otherwise lose up to frame_batch - 1 frames)
    if (!ctx->pending.empty() && hipSetDevice(ctx->device) == hipSuccess && flush_pending(ctx) != RTGL_OK)
        fprintf(stderr, "rtgl_destroy: %zu batched frame(s) could not be submitted: %s\n", ctx->pending.size(), ctx->error.c_str());
    unregister_ctx_stream(ctx);
    for (auto &w : ctx->workers) {
        { std::lock_guard<std::mutex> lk(w->m); w->state = PartWorker::kQuit; }
        w->cv.notify_all();
        if (w->th.joinable()) w->th.join();
    }
    ctx->workers.clear();
    for (rtgl_context *part : ctx->parts) rtgl_destroy(part);
    ctx->parts.clear();
    (void)hipSetDevice(ctx->device);
    for (hipEvent_t e : ctx->part_done) (void)hipEventDestroy(e);
    if (ctx->gather_done) (void)hipEventDestroy(ctx->gather_done);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
#ifdef RT_SOLO_STAMPS
    if (ctx->d_dbg_log) {      // diagnostics build: where the waves of the solo scan spent their cycles, per bounce, summed over all frames
        unsigned long long h[16 * 64];
        if (hipMemcpy(h, ctx->d_dbg_log, sizeof h, hipMemcpyDeviceToHost) == hipSuccess)
            for (int b = 0; b < 64 && h[16 * b + 8]; ++b) {
                const unsigned long long *d = h + 16 * b; const double tot = (double)d[0];
                fprintf(stderr, "rtgl stamps bounce %2d: waves %llu iters %llu  cycles/wave %.0f  staging %.1f%% rays %.1f%% segments %.1f%% (of the wave: set-up %.1f%%, park %.1f%%) flush %.1f%%  cycles per tile-stage in steady %.1f  slowest wave of a launch (mean over launches) %.0f  culled items %llu at %.0f cycles\n",
                        b, d[8], d[7], tot / d[8], 100.0 * d[1] / tot, 100.0 * d[2] / tot, 100.0 * d[4] / tot, 100.0 * d[3] / tot, 100.0 * d[5] / tot, 100.0 * d[6] / tot,
                        d[9] ? (double)d[4] / (double)d[9] : 0.0, (double)d[13] * (double)d[15] / (double)d[8], d[12], d[12] ? (double)d[11] / (double)d[12] : 0.0);
            }
#if RT_SOLO_STAMPS == 3
        if (hipMemcpy(h, ctx->d_dbg_log, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) {
            double cyc = 0, ticks = 0;
            for (int b = 0; b < 64 && h[16 * b + 8]; ++b) {
                const unsigned long long *d = h + 16 * b;
                fprintf(stderr, "rtgl clock bounce %2d: %llu waves, %.0f shader cycles per wave over %.0f ticks of 10 ns: %.3f GHz\n", b, d[8], (double)d[0] / d[8], (double)d[14] / d[8], d[14] ? (double)d[0] / (double)d[14] * 0.1 : 0.0);
                cyc += (double)d[0]; ticks += (double)d[14];
            }
            if (ticks > 0) fprintf(stderr, "rtgl clock: in-kernel shader clock of scan_solo_kernel, wave-time weighted over all launches: %.3f GHz\n", cyc / ticks * 0.1);
        }
#endif
        // the tail drain (narrow_fused): what the waves' regions held.  A window is 64 x 4 records; the per-record form takes 2 + (set bits of
        // the window's fullest mask) round trips for it, the pair form one per 256 pairs of the region
        unsigned long long dr[8 * 64];
        if (hipMemcpy(dr, reinterpret_cast<unsigned long long *>(ctx->d_dbg_log) + 1024, sizeof dr, hipMemcpyDeviceToHost) == hipSuccess)
            for (int b = 0; b < 64; ++b) {
                const unsigned long long *d = dr + 8 * b;
                if (!d[0]) continue;
                fprintf(stderr, "rtgl drain bounce %2d: regions %llu records %llu pairs %llu (%.3f per record)  windows %llu, fullest mask of a window %.2f bits: %.2f round trips per region by records, %.2f by pairs\n",
                        b, d[0], d[1], d[2], d[1] ? (double)d[2] / (double)d[1] : 0.0, d[3], d[3] ? (double)d[4] / (double)d[3] : 0.0,
                        (double)(2 * d[3] + d[4]) / (double)d[0], (double)d[5] / (double)d[0]);
            }
        // static launches: mean wave time per chunk, relative to the bounce's mean (what an uneven cost of the chunks loses)
        std::vector<unsigned long long> pc(16 * 64 * 2 * 16);
        if (hipMemcpy(pc.data(), reinterpret_cast<unsigned long long *>(ctx->d_dbg_log) + 2048, pc.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
            for (int b = 0; b < 8; ++b) {
                double tot = 0, cnt = 0; int nch = 0;
                for (int c = 0; c < 64; ++c) { const unsigned long long *e = pc.data() + ((size_t)16 * b * 64 + c) * 2; if (e[1]) { tot += (double)e[0]; cnt += (double)e[1]; nch = c + 1; } }
                if (cnt == 0) continue;
                fprintf(stderr, "rtgl stamps bounce %2d: mean wave time per chunk / bounce mean:", b);
                for (int c = 0; c < nch; ++c) { const unsigned long long *e = pc.data() + ((size_t)16 * b * 64 + c) * 2; fprintf(stderr, " %.2f", e[1] ? ((double)e[0] / (double)e[1]) / (tot / cnt) : 0.0); }
                fprintf(stderr, "\n");
            }
    }
#endif
    ctx->buffers.release_all();
    for (hipEvent_t e : ctx->kev) (void)hipEventDestroy(e);
    if (ctx->h_counts) (void)hipHostFree(ctx->h_counts);
    if (ctx->counts_ev) (void)hipEventDestroy(ctx->counts_ev);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->own_stream) release_device_stream(ctx->device, ctx->own_stream, ctx->own_stream_shared);
    delete ctx;
}

extern "C" const char *rtgl_last_error(const rtgl_context *ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

#define ENTER_NOFLUSH(ctx) do { if (!(ctx)) return RTGL_ERR_INVALID; HIPCHK(ctx, hipSetDevice((ctx)->device)); } while (0)
// every entry point but rtgl_render_frame / rtgl_set_frame_params first submits the frames a batching context is still holding back
#define ENTER(ctx) do { ENTER_NOFLUSH(ctx); if (!(ctx)->pending.empty()) { const int rcf_ = flush_pending(ctx); if (rcf_) return rcf_; } } while (0)
// multi-device context: run `call` on every part, report the first failure through the assembler
#define FANOUT(ctx, call) do { if (!(ctx)->parts.empty()) { (ctx)->gathered = false; \
    for (rtgl_context *part : (ctx)->parts) { const int rc_ = (call); if (rc_) return fail(ctx, rc_, std::string("device ") + std::to_string(part->device) + ": " + part->error); } \
    return RTGL_OK; } } while (0)

// ---- single-process multi-device context (create(w, h, devices[], n)) --------------------------------------------
// Replaces the ONE glDispatchCompute of the reference (src/renderer.cpp:129-134) by one strip-tiled dispatch per device; the tile
// buffers are gathered to devices[0] over xGMI (peer copies, one 2-D copy per part: strips of a part are `world` strips apart in
// the assembled image) when the image is consumed.  The same device may be listed more than once (several contexts on one GPU).
extern "C" int rtgl_create_multi(rtgl_context **out, int width, int height, const int *devices, int n_devices, int strip_rows)
{
    if (!out) return fail(nullptr, RTGL_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!devices || n_devices < 1 || n_devices > 64) return fail(nullptr, RTGL_ERR_INVALID, "rtgl_create_multi: need 1..64 device ordinals");
    rtgl_context *ctx = nullptr;
    int rc = rtgl_create_tiled(&ctx, width, height, devices[0], 0, 1, strip_rows);         // the assembler: full image on devices[0]
    if (rc) return rc;
    for (int i = 0; i < n_devices; ++i) {
        rtgl_context *part = nullptr;
        rc = rtgl_create_tiled(&part, width, height, devices[i], i, n_devices, strip_rows);
        if (rc) { const std::string msg = g_create_error; rtgl_destroy(ctx); g_create_error = msg; return rc; }
        // (parts that share a device share its stream, like all contexts of the process: acquire_device_stream)
        ctx->parts.push_back(part);
        hipEvent_t ev = nullptr;
        (void)hipSetDevice(devices[i]);
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { rtgl_destroy(ctx); return fail(nullptr, RTGL_ERR_DEVICE, "hipEventCreate failed"); }
        ctx->part_done.push_back(ev);
        if (devices[i] != devices[0]) {           // xGMI peer copies; without peer access the gather goes through the host
            int can = 0;
            (void)hipSetDevice(devices[0]);
            if (hipDeviceCanAccessPeer(&can, devices[0], devices[i]) != hipSuccess || !can) ctx->peer_copy = false;
            else { hipError_t e = hipDeviceEnablePeerAccess(devices[i], 0); if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) ctx->peer_copy = false; }
            (void)hipGetLastError();
        }
    }
    const char *mt = getenv("RTGL_AMD_MULTI_THREADS");
    if (n_devices > 1 && !(mt && atoi(mt) == 0)) try {
        for (rtgl_context *part : ctx->parts) {
            ctx->workers.emplace_back(new PartWorker);
            PartWorker *w = ctx->workers.back().get();
            w->part = part;
            w->th = std::thread([w] {
                std::unique_lock<std::mutex> lk(w->m);
                for (;;) {
                    w->cv.wait(lk, [w] { return w->state == PartWorker::kJob || w->state == PartWorker::kQuit; });
                    if (w->state == PartWorker::kQuit) return;
                    lk.unlock();
                    const int rc = rtgl_render_frame(w->part);      // (sets the thread's device itself: ENTER)
                    lk.lock();
                    w->rc = rc; w->state = PartWorker::kDone;
                    w->cv.notify_all();
                }
            });
        }
    } catch (const std::exception &) {                   // no threads to be had: the caller's thread submits, as with RTGL_AMD_MULTI_THREADS=0
        for (auto &w : ctx->workers) {
            { std::lock_guard<std::mutex> lk(w->m); w->state = PartWorker::kQuit; }
            w->cv.notify_all();
            if (w->th.joinable()) w->th.join();
        }
        ctx->workers.clear();
    }
    *out = ctx;
    return RTGL_OK;
}

extern "C" int rtgl_device_count(const rtgl_context *ctx) { return ctx ? (ctx->parts.empty() ? 1 : (int)ctx->parts.size()) : RTGL_ERR_INVALID; }

// strips of every part -> the assembler's image (global row order), on the assembler's stream, after each part's queued frames
static int multi_gather(rtgl_context *ctx)
{
    if (ctx->gathered) return RTGL_OK;
    const int world = (int)ctx->parts.size(), sr = ctx->strip_rows;
    const size_t row_bytes = (size_t)ctx->width * 16, strip_bytes = row_bytes * sr;
    std::vector<float> host;
    for (int i = 0; i < world; ++i) {
        rtgl_context *part = ctx->parts[i];
        if (!part->pending.empty()) { HIPCHK(ctx, hipSetDevice(part->device)); const int rc = flush_pending(part); if (rc) return fail(ctx, rc, part->error); }
        const int full = part->local_rows / sr, tail_rows = part->local_rows - full * sr;       // only the owner of the last strip has a short one
        uint8_t *dst = reinterpret_cast<uint8_t *>(ctx->d_image) + (size_t)i * strip_bytes;
        const uint8_t *src = reinterpret_cast<const uint8_t *>(part->d_image);
        if (ctx->peer_copy) {
            HIPCHK(ctx, hipSetDevice(part->device));
            HIPCHK(ctx, hipEventRecord(ctx->part_done[i], part->stream));
            HIPCHK(ctx, hipSetDevice(ctx->device));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->part_done[i], 0));
            if (full) HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)world * strip_bytes, src, strip_bytes, strip_bytes, (size_t)full, hipMemcpyDeviceToDevice, ctx->stream));
            if (tail_rows) HIPCHK(ctx, hipMemcpyAsync(dst + (size_t)full * world * strip_bytes, src + (size_t)full * strip_bytes, row_bytes * tail_rows, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            host.resize((size_t)part->local_rows * ctx->width * 4);
            int rc = rtgl_read_image_f32(part, host.data());
            if (rc) return fail(ctx, rc, part->error);
            HIPCHK(ctx, hipSetDevice(ctx->device));
            if (full) HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)world * strip_bytes, host.data(), strip_bytes, strip_bytes, (size_t)full, hipMemcpyHostToDevice, ctx->stream));
            if (tail_rows) HIPCHK(ctx, hipMemcpyAsync(dst + (size_t)full * world * strip_bytes, reinterpret_cast<const uint8_t *>(host.data()) + (size_t)full * strip_bytes, row_bytes * tail_rows, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->peer_copy) {
        // the copies read every part's tile buffer on the ASSEMBLER's stream: the parts' next frames (their own streams) must not overwrite
        // the tiles before the copies are through
        if (!ctx->gather_done) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->gather_done, hipEventDisableTiming));
        HIPCHK(ctx, hipEventRecord(ctx->gather_done, ctx->stream));
        for (rtgl_context *part : ctx->parts)
            if (part->stream != ctx->stream) {
                HIPCHK(ctx, hipSetDevice(part->device));
                HIPCHK(ctx, hipStreamWaitEvent(part->stream, ctx->gather_done, 0));
            }
        HIPCHK(ctx, hipSetDevice(ctx->device));
    }
    ctx->gathered = true;
    return RTGL_OK;
}

extern "C" int rtgl_gather_tiles(rtgl_context *ctx)
{
    ENTER(ctx);
    if (ctx->parts.empty()) return RTGL_OK;            // a single-device context holds its image already
    return multi_gather(ctx);
}

extern "C" int rtgl_upload_spheres(rtgl_context *ctx, const void *data, uint32_t count)
{
    ENTER(ctx);
    FANOUT(ctx, rtgl_upload_spheres(part, data, count));
    if (count && !data) return fail(ctx, RTGL_ERR_INVALID, "spheres is NULL");
    static_assert(sizeof(SphereRec) == 32, "Sphere stride (shaders/raytracer.glsl:11-15, std140)");
    int rc = realloc_upload(ctx, ctx->d_spheres, data, (size_t)count * 32);
    if (rc) return rc;
    ctx->n_spheres = count; ctx->visits_dirty = true;
    return RTGL_OK;
}

extern "C" int rtgl_upload_materials(rtgl_context *ctx, const void *data, uint32_t count)
{
    ENTER(ctx);
    FANOUT(ctx, rtgl_upload_materials(part, data, count));
    if (count && !data) return fail(ctx, RTGL_ERR_INVALID, "materials is NULL");
    static_assert(sizeof(MaterialRec) == 32, "Material stride (shaders/raytracer.glsl:17-21, std140)");
    int rc = realloc_upload(ctx, ctx->d_materials, data, (size_t)count * 32);
    if (rc) return rc;
    ctx->n_materials = count;
    return RTGL_OK;
}

extern "C" int rtgl_upload_meshes(rtgl_context *ctx, const void *data, uint32_t count)
{
    ENTER(ctx);
    FANOUT(ctx, rtgl_upload_meshes(part, data, count));
    if (count && !data) return fail(ctx, RTGL_ERR_INVALID, "meshes is NULL");
    ctx->h_meshes.assign((const uint8_t *)data, (const uint8_t *)data + (size_t)count * 16);
    ctx->n_meshes = count; ctx->tris_dirty = true;
    return RTGL_OK;
}

extern "C" int rtgl_upload_vertices(rtgl_context *ctx, const void *data, uint32_t vec4_count)
{
    ENTER(ctx);
    FANOUT(ctx, rtgl_upload_vertices(part, data, vec4_count));
    if (vec4_count && !data) return fail(ctx, RTGL_ERR_INVALID, "vertices is NULL");
    int rc = realloc_upload(ctx, ctx->d_vertices, data, (size_t)vec4_count * 16);
    if (rc) return rc;
    ctx->h_vertices.assign((const uint8_t *)data, (const uint8_t *)data + (size_t)vec4_count * 16);   // host copy: spatial ordering of the triangles
    ctx->n_vec4 = vec4_count; ctx->tris_dirty = true;
    return RTGL_OK;
}

extern "C" int rtgl_upload_nodes(rtgl_context *ctx, const void *data, uint32_t count)
{
    ENTER(ctx);
    FANOUT(ctx, rtgl_upload_nodes(part, data, count));
    if (count && !data) return fail(ctx, RTGL_ERR_INVALID, "nodes is NULL");
    ctx->h_nodes.assign((const uint8_t *)data, (const uint8_t *)data + (size_t)count * 48);
    ctx->n_nodes = count; ctx->visits_dirty = true;
    return RTGL_OK;
}

extern "C" int rtgl_upload_envmap(rtgl_context *ctx, const uint8_t *faces, int nfaces, int width, int height, int channels)
{
    ENTER(ctx);
    FANOUT(ctx, rtgl_upload_envmap(part, faces, nfaces, width, height, channels));
    if (nfaces < 0 || nfaces > 6 || width <= 0 || height <= 0 || (channels != 3 && channels != 4) || (nfaces && !faces))
        return fail(ctx, RTGL_ERR_INVALID, "envmap: need 0..6 faces, positive size, 3 or 4 channels");
    int rc = realloc_upload(ctx, ctx->d_env, faces, (size_t)nfaces * width * height * channels);
    if (rc) return rc;
    ctx->env_w = width; ctx->env_h = height; ctx->env_c = channels; ctx->env_faces = nfaces;
    return RTGL_OK;
}

// traverse() (:272-329) walks the node buffer identically for every ray; run that walk once here (rt_node_walk.hpp holds the rules) and
// keep the sphere indices in test order.
static_assert(rt_node_walk::kNoSphereVisit == kNoSphere, "the walk and the sphere scan name the zero sphere alike");
static int rebuild_sphere_visits(rtgl_context *ctx)
{
    std::vector<uint32_t> visits;
    const size_t kMaxVisits = 1u << 20;
    if (!rt_node_walk::walk(ctx->h_nodes.data(), ctx->n_nodes, ctx->n_spheres, kMaxVisits, visits))
        return fail(ctx, RTGL_ERR_INVALID, "node buffer expands to more than 2^20 sphere tests per ray");
    int rc = realloc_upload(ctx, ctx->d_sphere_visits, visits.data(), visits.size() * sizeof(uint32_t));
    if (rc) return rc;
    ctx->n_sphere_visits = (uint32_t)visits.size();
    ctx->visits_dirty = false;
    return RTGL_OK;
}

// Storage order of the triangle visits for the matrix-core broad phase: the leaves of a k-d tree (median split along the longest axis),
// written out left to right.  A leaf is one MFMA tile (10 triangles); the split positions are multiples of the unit above them (tile ->
// quad of 4 tiles -> group of `group_tris` triangles), so every tile, quad and group of the storage order is one subtree.
//   * down to the groups the tree splits the triangle CENTROIDS: a group shares one local origin and one set of bounds in the bf16
//     broad phase (rt_mfma.hpp), whose margin grows with the group's extent;
//   * inside a group it splits the six-dimensional points (centroid, lambda x unit normal), lambda = 0.4 x the mesh's extent: a
//     tile's culling record (rt_mfma.hpp, MfCull) bounds its ten normals by a rectangle, and on a mesh that is coarse against its own
//     curvature (the 100,000-triangle benchmark field turns by 15 degrees from one cell to the next) ten NEIGHBOURS spread +-33 degrees --
//     a quarter of all far tiles then fail the certificates on their normals alone.  Ten triangles of similar slope from anywhere in
//     the group (3 units across there) spread +-9 degrees; that the tile's sphere grows from 0.5 to 1.5 units costs far less
//     (emulated on real bounce-1 rays, tools/diagnostics/cull_emulation.py: 49 -> 64 % of the tile tests certified at 100k triangles,
//     88 -> 97 % on its camera bounce; 67 -> 70 % and 99.6 -> 98.9 % at 10k).
// Only tightness depends on the order: hits merge by VISIT index.  Non-finite centroids and degenerate normals sort as 0.
// Deterministic: ties break by visit index.
static std::vector<uint32_t> kd_order(const rtgl_context *ctx, const std::vector<uint32_t> &visit_tri, uint32_t group_tris)
{
    const size_t n = visit_tri.size();
    const float *vx = reinterpret_cast<const float *>(ctx->h_vertices.data());
    std::vector<float> pts(6 * n);
    float blo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, bhi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    auto finite = [](float c) { return c == c && c > -1.0e30f && c < 1.0e30f; };
    for (size_t v = 0; v < n; ++v) {
        const float *t = vx + (size_t)visit_tri[v] * 12;
        for (int a = 0; a < 3; ++a) {
            const float c = (t[a] + t[4 + a] + t[8 + a]) * (1.0f / 3.0f);
            pts[6 * v + a] = finite(c) ? c : 0.0f;
            if (finite(c)) { blo[a] = std::min(blo[a], c); bhi[a] = std::max(bhi[a], c); }
        }
        const float e1[3] = {t[4] - t[0], t[5] - t[1], t[6] - t[2]}, e2[3] = {t[8] - t[0], t[9] - t[1], t[10] - t[2]};
        const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        const float nl = std::sqrt(nx * nx + ny * ny + nz * nz);
        const bool ok = finite(nl) && nl > 0.0f;
        pts[6 * v + 3] = ok ? nx / nl : 0.0f; pts[6 * v + 4] = ok ? ny / nl : 0.0f; pts[6 * v + 5] = ok ? nz / nl : 0.0f;
    }
    float ext = 0.0f;
    for (int a = 0; a < 3; ++a) if (blo[a] <= bhi[a]) ext = std::max(ext, bhi[a] - blo[a]);
    float lambda = 0.4f * ext;
    // (tuning: fraction of the mesh's extent.  The weight only orders the triangles into tiles -- every bound is taken over what a tile
    // ends up holding, so any order is a correct one -- but the splits below compare the weighted normals, and a NaN or an
    // infinite weight (0 x inf) would hand nth_element keys without a strict weak order: finite values of 0 .. 1e6 only, else the default)
    if (const char *e = getenv("RTGL_AMD_KD_LAMBDA")) { const float v = (float)atof(e); if (std::isfinite(v) && v >= 0.0f && v <= 1.0e6f) lambda = v * ext; }
    for (size_t v = 0; v < n; ++v) for (int a = 3; a < 6; ++a) pts[6 * v + a] *= lambda;
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::vector<std::pair<size_t, size_t>> todo;
    if (n) todo.emplace_back(0, n);
    while (!todo.empty()) {
        const size_t lo = todo.back().first, hi = todo.back().second, m = hi - lo;
        todo.pop_back();
        if (m <= (size_t)kMfTileTris) continue;
        const size_t unit = m > group_tris ? group_tris : (m > (size_t)kMfQuadTris ? (size_t)kMfQuadTris : (size_t)kMfTileTris);
        const size_t nl = ((m / 2 + unit - 1) / unit) * unit;           // in [unit, m): m > unit
        const int dims = m > group_tris ? 3 : 6;
        float bl[6], bh[6];
        for (int a = 0; a < dims; ++a) { bl[a] = 3.0e38f; bh[a] = -3.0e38f; }
        for (size_t i = lo; i < hi; ++i)
            for (int a = 0; a < dims; ++a) { const float c = pts[6 * (size_t)order[i] + a]; bl[a] = std::min(bl[a], c); bh[a] = std::max(bh[a], c); }
        int ax = 0;
        for (int a = 1; a < dims; ++a) if (bh[a] - bl[a] > bh[ax] - bl[ax]) ax = a;
        std::nth_element(order.begin() + lo, order.begin() + lo + nl, order.begin() + hi, [&](uint32_t p, uint32_t q) {
            const float cp = pts[6 * (size_t)p + ax], cq = pts[6 * (size_t)q + ax];
            return cp < cq || (cp == cq && p < q);
        });
        todo.emplace_back(lo, lo + nl);
        todo.emplace_back(lo + nl, hi);
    }
    return order;
}

// Packet culling in nodes of 4, 16 or 64 tiles (rt_scan.hpp, packet_cull_kernel) or tile by tile (0).  Tuning switch RTGL_AMD_CULL_NODE =
// 0 or the node size; other sizes are taken to the nearest valid one.  Read when the triangles are uploaded (the node records are built then).
static uint32_t cull_node_shift_option()
{
    uint32_t shift = 4;
    if (const char *e = getenv("RTGL_AMD_CULL_NODE")) { const long v = atol(e); shift = v <= 0 ? 0u : v <= 8 ? 2u : v <= 32 ? 4u : 6u; }      // (tuning)
    return shift;
}

static int rebuild_triangles(rtgl_context *ctx)
{
    std::vector<uint32_t> visit_tri, visit_mesh;
    uint32_t n_tris = ctx->n_vec4 / 3;   // to_triangles() drops a trailing partial triangle (src/renderer.h:34-48)
    rt_mesh_visits::expand(ctx->h_meshes.data(), ctx->n_meshes, n_tris, visit_mesh, visit_tri);      // the shader's 32-bit loop bounds
    ctx->h_visit_tri = visit_tri; ctx->h_visit_mesh.swap(visit_mesh); ctx->visit_ids_dirty = true;      // (the ids plane's triangle ids)
    RCCHK(buf_release(ctx, ctx->d_edges, ctx->d_planes));
    ctx->n_tri_visits = (uint32_t)visit_tri.size();
    ctx->scene_version++;
    {
        float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
        const float *vx = reinterpret_cast<const float *>(ctx->h_vertices.data());
        for (uint32_t t : visit_tri)
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) { const float c = vx[(size_t)t * 12 + 4 * k + a]; if (c == c && c > -1.0e30f && c < 1.0e30f) { lo[a] = std::min(lo[a], c); hi[a] = std::max(hi[a], c); } }
        ctx->mesh_ext = 0.0f;
        for (int a = 0; a < 3; ++a) { ctx->mesh_lo[a] = lo[a] <= hi[a] ? lo[a] : 0.0f; ctx->mesh_hi[a] = lo[a] <= hi[a] ? hi[a] : 0.0f; if (lo[a] <= hi[a]) ctx->mesh_ext = std::max(ctx->mesh_ext, hi[a] - lo[a]); }
    }
    if (ctx->n_tri_visits) {
        RCCHK(buf_alloc(ctx, ctx->d_visit_scratch, visit_tri.size() * 4));
        uint32_t *const d_visit = ctx->d_visit_scratch;
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_visit_scratch, visit_tri.data(), visit_tri.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        RCCHK(buf_alloc(ctx, ctx->d_edges, (size_t)ctx->n_tri_visits * sizeof(TriEdges)));
        RCCHK(buf_alloc(ctx, ctx->d_planes, (size_t)ctx->n_tri_visits * sizeof(TriPlane)));
        dim3 grid((ctx->n_tri_visits + 255) / 256);
        hipLaunchKernelGGL(prepare_triangles_kernel, grid, dim3(256), 0, ctx->stream, ctx->d_vertices, d_visit, ctx->n_tri_visits, ctx->d_edges, ctx->d_planes);
        HIPCHK(ctx, hipGetLastError());
        uint32_t n_groups = (ctx->n_tri_visits + kBoundGroup - 1) / kBoundGroup;
        RCCHK(buf_alloc(ctx, ctx->d_group_bounds, (size_t)n_groups * sizeof(float2)));
        hipLaunchKernelGGL(group_bounds_kernel, dim3(n_groups), dim3(64), 0, ctx->stream, ctx->d_edges, ctx->n_tri_visits, ctx->d_group_bounds);
        HIPCHK(ctx, hipGetLastError());
        // bf16 broad-phase data: local origins, bounds, A matrices (rt_mfma.hpp)
        RCCHK(buf_release(ctx, ctx->d_mf_groups, ctx->d_mf_A, ctx->d_mf_order, ctx->d_mf_cull, ctx->d_mf_cull_node, ctx->d_edges_s, ctx->d_planes_s));
        // quads sharing one local origin: 32 (= a chunk: one ray set-up per work item of the scan) unless the caller chose.  Smaller
        // groups have tighter bounds and fewer survivors (C4: 89 M per frame at 8 quads against 111 M at 32), but every group of a
        // chunk costs the scan a ray set-up and a pipeline fill of its own: 28.4 against 30.0 Mpaths/s
        ctx->mf_group_quads = ctx->group_explicit ? (uint32_t)ctx->opt.mf_group_quads : 32u;
        const uint32_t group_tris = ctx->mf_group_quads * kMfQuadTris;
        ctx->n_mf_groups = (ctx->n_tri_visits + group_tris - 1) / group_tris;
        const std::vector<uint32_t> order = kd_order(ctx, visit_tri, group_tris);
        RCCHK(buf_alloc(ctx, ctx->d_mf_order, order.size() * 4));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_mf_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        RCCHK(buf_alloc(ctx, ctx->d_edges_s, (size_t)ctx->n_tri_visits * sizeof(TriEdges)));
        RCCHK(buf_alloc(ctx, ctx->d_planes_s, (size_t)ctx->n_tri_visits * sizeof(TriPlane)));
        hipLaunchKernelGGL(gather_storage_order_kernel, dim3((ctx->n_tri_visits + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_edges, ctx->d_planes, ctx->d_mf_order,
                           ctx->n_tri_visits, ctx->d_edges_s, ctx->d_planes_s);
        RCCHK(buf_alloc(ctx, ctx->d_mf_groups, (size_t)ctx->n_mf_groups * sizeof(MfGroup)));
        const size_t a_bytes = ((size_t)ctx->n_mf_groups * ctx->mf_group_quads + 1) * kMfQuadTiles * 64 * sizeof(uint4);   // two K panels per tile; + one zero quad
        if (a_bytes > 0xFFFF0000ull) return fail(ctx, RTGL_ERR_INVALID, "mesh too large for the 32-bit tile offsets of the matrix-core scan");
        RCCHK(buf_alloc(ctx, ctx->d_mf_A, a_bytes));
        HIPCHK(ctx, hipMemsetAsync(ctx->d_mf_A, 0, a_bytes, ctx->stream));
        hipLaunchKernelGGL(prepare_mfma_kernel, dim3(ctx->n_mf_groups), dim3(64), 0, ctx->stream, ctx->d_vertices, d_visit,
                           ctx->d_mf_order, ctx->n_tri_visits, ctx->n_mf_groups, ctx->mf_group_quads, ctx->d_mf_groups, ctx->d_mf_A, getenv("RTGL_AMD_ROW_GAMMA") ? (float)atof(getenv("RTGL_AMD_ROW_GAMMA")) : 1.220703125e-4f);      // (tuning.  Any value is covered: it only picks the row's scale, which mf_build_rows_kernel takes as a power of two within 1e-12 .. 1e12 or as 1 -- exact either way, and the group's bounds are taken over the scaled rows: DESIGN.md 3.1)
        HIPCHK(ctx, hipGetLastError());
        // packet-culling records, one per tile of the storage order (all-zero records -- unusable -- behind the last one)
        const uint32_t n_tiles_all = ctx->n_mf_groups * ctx->mf_group_quads * (uint32_t)kMfQuadTiles, n_tiles_alloc = n_tiles_all + 128u;
        RCCHK(buf_alloc(ctx, ctx->d_mf_cull, (size_t)n_tiles_alloc * sizeof(MfCull)));
        HIPCHK(ctx, hipMemsetAsync(ctx->d_mf_cull, 0, (size_t)n_tiles_alloc * sizeof(MfCull), ctx->stream));
        hipLaunchKernelGGL(prepare_cull_kernel, dim3(n_tiles_all), dim3(64), 0, ctx->stream, ctx->d_vertices, d_visit,
                           ctx->d_mf_order, ctx->n_tri_visits, n_tiles_all, (uint32_t)kMfTileTris, ctx->d_mf_cull);
        HIPCHK(ctx, hipGetLastError());
        // ... and one per node of 2^cull_node_shift consecutive tiles (packet_cull_kernel, pass 1)
        ctx->cull_node_shift = cull_node_shift_option();
        if (ctx->cull_node_shift) {
            const uint32_t n_nodes_all = (n_tiles_all + (1u << ctx->cull_node_shift) - 1u) >> ctx->cull_node_shift;
            RCCHK(buf_alloc(ctx, ctx->d_mf_cull_node, (size_t)n_nodes_all * sizeof(MfCull)));
            hipLaunchKernelGGL(prepare_cull_kernel, dim3(n_nodes_all), dim3(64), 0, ctx->stream, ctx->d_vertices, d_visit,
                               ctx->d_mf_order, ctx->n_tri_visits, n_nodes_all, (uint32_t)kMfTileTris << ctx->cull_node_shift, ctx->d_mf_cull_node);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        RCCHK(buf_release(ctx, ctx->d_visit_scratch));
    } else ctx->n_mf_groups = 0;
    ctx->tris_dirty = false;
    return RTGL_OK;
}

// event pair around one dominant-kernel launch (only with option kernel_timing)
static void kev_mark(rtgl_context *ctx)
{
    if (!ctx->timing_this_frame) return;
    if (ctx->kev_used == ctx->kev.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; ctx->kev.push_back(e); }
    (void)hipEventRecord(ctx->kev[ctx->kev_used++], ctx->stream);
}

// ---- bounce-wavefront pipeline: buffers + launches ------------------------------------------------
// the scan launch policy (rt_scan_launch.hpp): what it needs to know of the device, the mesh and the options
static_assert(rt_scan_launch::kQuadTris == (uint32_t)kMfQuadTris && rt_scan_launch::kQuadTiles == (uint32_t)kMfQuadTiles && rt_scan_launch::kRaysPerWave == SoloCfg::kRaysPerWave, "rt_scan_launch.hpp");
static rt_scan_launch::Setup scan_setup(const rtgl_context *ctx) { return {(uint32_t)ctx->n_cus, rt_scan_launch::real_quads(ctx->n_mf_groups, ctx->mf_group_quads, ctx->n_tri_visits), (uint32_t)ctx->opt.mf_chunk_quads, ctx->opt.scan_waves, ctx->opt.scan_dynamic, ctx->opt.cull}; }

static size_t counts_bytes(uint32_t capacity) { return (size_t)(capacity + 1u) * sizeof(uint32_t); }      // ray counts per bounce + the fullest candidate region

// The environment's tuning of ray binning.  A refused (RTGL_AMD_SORT_OB, RTGL_AMD_SORT_DB) pair falls back to the defaults with one line on
// stderr (tuning variables have no status path); rt_bin_plan.hpp says which pairs are accepted and why.
static rt_bin_plan::Plan bin_plan(rtgl_context *ctx, uint32_t n0)
{
    const char *eo = getenv("RTGL_AMD_SORT_OB"), *ed = getenv("RTGL_AMD_SORT_DB");
    const rt_bin_plan::Plan p = rt_bin_plan::plan(n0, eo ? std::max(atoi(eo), 0) : -1, ed ? std::max(atoi(ed), 0) : -1);
    if (p.refused && !ctx->bin_refusal_said) {                // (once per context)
        fprintf(stderr, "rtgl_amd: RTGL_AMD_SORT_OB=%s RTGL_AMD_SORT_DB=%s refused (rt_bin_plan.hpp: accepted pairs), using %u and %u\n", eo ? eo : "(unset)", ed ? ed : "(unset)", p.ob, p.db);
        ctx->bin_refusal_said = true;
    }
    return p;
}

// The cells of the bin key's origin word (rt_bin_plan::cells) for the mesh in place
static void set_bin_cells(rtgl_context *ctx, const rt_bin_plan::Plan &plan)
{
    const char *es = getenv("RTGL_AMD_BIN_SPLIT"), *eu = getenv("RTGL_AMD_BIN_UNIT");      // (tuning: 0 = every origin clamped into the box's cells; the outside cells' unit)
    ctx->wb.sort_cells = rt_bin_plan::cells(ctx->mesh_lo, ctx->mesh_hi, ctx->mesh_ext, plan.T, plan.db, !(es && atoi(es) == 0), eu ? (float)atof(eu) : 0.0f);
}

static int ensure_wave_buffers(rtgl_context *ctx, uint32_t n0, uint32_t max_bounce, bool multi_sample)
{
    if (ctx->counts_capacity < max_bounce + 2) {
        ctx->counts_capacity = 0;                            // (non-zero only while BOTH buffers are live with that capacity)
        RCCHK(buf_alloc(ctx, ctx->d_counts, counts_bytes(max_bounce + 2)));                                     // u32 ray counts per bounce
        if (ctx->h_counts) { HIPCHK(ctx, hipHostFree(ctx->h_counts)); ctx->h_counts = nullptr; }
        HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_counts, counts_bytes(max_bounce + 2), hipHostMallocDefault));
        if (!ctx->counts_ev) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->counts_ev, hipEventDisableTiming));
        ctx->counts_capacity = max_bounce + 2; ctx->counts_pending = ctx->counts_valid = false; ctx->est_counts.clear();
    }
    if (ctx->opt.kernel == RTGL_KERNEL_WAVEFRONT_MFMA_SOLO) {
        const rt_scan_launch::Capacity scan = rt_scan_launch::capacity(scan_setup(ctx));
        const uint32_t need_regions = scan.regions;
        // (a record = one (ray, 5-triangle mask); every queue entry of the scan makes four of them)
        if (!ctx->cand_region_target) ctx->cand_region_target = std::max<uint32_t>(4096u, (uint32_t)std::min<uint64_t>(((uint64_t)n0 + need_regions - 1) / need_regions, 0xFFFFFFF0u));
        if (!ctx->d_cand || need_regions > ctx->cand_regions || ctx->cand_region_target > ctx->cand_region_pairs) {
            ctx->cand_regions = need_regions; ctx->cand_region_pairs = ctx->cand_region_target;
            RCCHK(buf_alloc(ctx, ctx->d_cand, ((size_t)need_regions * ctx->cand_region_pairs) * sizeof(uint2) + (size_t)need_regions * sizeof(uint32_t) + 256));      // (the free waits for the frames in flight)
        }
        // packet culling: the keep bits of the queue being scanned; work distribution of the scan: one counter per (bounce, chunk)
        const size_t need_keep = scan.keep_count(n0), need_sched = (size_t)(max_bounce + 2) * scan.sched_stride;
        RCCHK(buf_grow(ctx, ctx->d_keep, ctx->keep_capacity, need_keep, need_keep * sizeof(uint32_t)));
        RCCHK(buf_grow(ctx, ctx->d_sched, ctx->sched_capacity, need_sched, need_sched * sizeof(uint32_t)));
        ctx->wb.keep_words = scan.keep_words; ctx->wb.keep = ctx->d_keep; ctx->wb.sched_stride = scan.sched_stride; ctx->wb.sched = ctx->d_sched;
        if (ctx->opt.cull == 3) {                            // ray binning: staging queue (64-byte records of a, b, c, rng, pixel 4 B), key + rank 8 B, source slot 4 B, and the bin counters
            RCCHK(buf_grow(ctx, ctx->d_stage, ctx->stage_capacity, n0, (size_t)n0 * 80 + 1024));
            uint8_t *p = (uint8_t *)ctx->d_stage;
            const size_t cap = ctx->stage_capacity;
            ctx->wb.stage = (float4 *)p; p += cap * 64; ctx->wb.sort_kr = (uint2 *)p; p += cap * 8; ctx->wb.stage_pixel = (uint32_t *)p; p += cap * 4;
            ctx->wb.sort_src = (uint32_t *)p;
            // (C5, 8.3 M rays: 917 Mpaths/s with 4 origin bit triples, 909 with 5; C2 in batches of eight, 16.6 M: 2.12 against 2.10 ms per frame)
            const rt_bin_plan::Plan plan = bin_plan(ctx, n0);
            ctx->wb.sort_ob = plan.ob; ctx->wb.sort_bits = plan.bits;
            if (ctx->sort_bits_alloc < ctx->wb.sort_bits) ctx->sort_sets_clean = false;
            RCCHK(buf_grow(ctx, ctx->d_sort_hist, ctx->sort_bits_alloc, ctx->wb.sort_bits, rt_bin_plan::hist_words(plan) * sizeof(uint32_t)));
            ctx->wb.sort_hist = ctx->d_sort_hist; ctx->wb.sort_hist_other = ctx->d_sort_hist;      // (set per binned bounce: launch_wavefront)
            set_bin_cells(ctx, plan);
        }
        ctx->wb.hybrid_div = rt_scan_items::kHybridDivDefault;          // (measured on C2 / C5: every 7th claimed 707 / 752 Mpaths/s, every 3rd 720 / 776, every 2nd 724 / 777, all of them 677 / 737;
                                                                        // the "every 2nd" figures were taken while a wave could reuse a record of its turns in the tail at that
                                                                        // setting (one granule scanned twice, one never: rt_scan_items.hpp) -- unverified since)
        if (const char *e = getenv("RTGL_AMD_HYBRID_DIV")) { const long v = atol(e); if (rt_scan_items::hybrid_div_accepted(v)) ctx->wb.hybrid_div = (uint32_t)v; }      // (tuning)
        ctx->wb.items = reinterpret_cast<uint32_t *>(ctx->d_items); ctx->wb.item_counts = reinterpret_cast<uint32_t *>(ctx->d_items);     // (allocated by the first culled launch)
        ctx->wb.cand = ctx->d_cand;
        ctx->wb.cand_counts = reinterpret_cast<uint32_t *>(ctx->d_cand + (size_t)ctx->cand_regions * ctx->cand_region_pairs);
        ctx->wb.cand_region = ctx->cand_region_pairs;
        // diagnostics: RTGL_DEBUG_CAND_CAP=n pretends a wave's region holds n pairs only, so that the in-place fallback of the scan runs
        if (const char *cc = getenv("RTGL_DEBUG_CAND_CAP")) { ctx->wb.cand_region = std::min<uint32_t>(ctx->wb.cand_region, (uint32_t)atoi(cc)); ctx->cand_fixed = true; }
    }
    if (multi_sample && !ctx->wave_multi) ctx->wave_capacity = 0;      // (the buffer in place lacks the per-pixel state)
    if (ctx->wave_capacity < n0) {
        // per queue: 4 x 16 B + 4 B per ray; per-pixel state for u_samples > 1: 4 x 16 B
        const size_t px = local_px(ctx), q_bytes = (size_t)n0 * (68 + 8), bytes = 2 * q_bytes + 1024 + (multi_sample ? px * 64 : 0);
        RCCHK(buf_grow(ctx, ctx->d_wave, ctx->wave_capacity, n0, bytes));
        ctx->wave_multi = multi_sample;
        uint8_t *p = (uint8_t *)ctx->d_wave;
        for (int q = 0; q < 2; ++q) {
            ctx->wb.q[q].a = (float4 *)p; p += (size_t)n0 * 16;
            ctx->wb.q[q].b = (float4 *)p; p += (size_t)n0 * 16;
            ctx->wb.q[q].c = (float4 *)p; p += (size_t)n0 * 16;
            ctx->wb.q[q].rng = (uint4 *)p; p += (size_t)n0 * 16;
        }
        for (int q = 0; q < 2; ++q) { ctx->wb.best[q] = (unsigned long long *)p; p += (size_t)n0 * 8; }
        for (int q = 0; q < 2; ++q) { ctx->wb.q[q].pixel = (uint32_t *)p; p += (size_t)n0 * 4; }
        p = (uint8_t *)(((uintptr_t)p + 255) & ~(uintptr_t)255);
        if (multi_sample) {
            ctx->wb.sums = (float4 *)p; p += px * 16;
            ctx->wb.cam_a = (float4 *)p; p += px * 16;
            ctx->wb.cam_b = (float4 *)p; p += px * 16;
            ctx->wb.pix_rng = (uint4 *)p; p += px * 16;
        } else ctx->wb.sums = ctx->wb.cam_a = ctx->wb.cam_b = nullptr, ctx->wb.pix_rng = nullptr;
    }
    ctx->wb.counts = ctx->d_counts;
    ctx->wb.cand_peak = ctx->d_counts + ctx->counts_capacity;
    ctx->wb.group_bounds = ctx->d_group_bounds;
    return RTGL_OK;
}

// aov != NULL: the launch of bounce 0 of sample 0 with option "aov" on (the instance that also writes the first-hit planes)
template <int R, int MODE>
static void launch_bounce(rtgl_context *ctx, const SceneView &sc, const FrameParams &P, const ImageView &im, uint32_t n0, uint32_t bounce, uint4 *rng_out, const AovView *aov)
{
    dim3 grid((n0 + 256u * R - 1) / (256u * R));
    if (aov) {
        if (ctx->opt.counters) hipLaunchKernelGGL((bounce_kernel<R, MODE, true, true>), grid, dim3(256), 0, ctx->stream, sc, P, im, ctx->wb, bounce, rng_out, ctx->d_counters, *aov);
        else hipLaunchKernelGGL((bounce_kernel<R, MODE, false, true>), grid, dim3(256), 0, ctx->stream, sc, P, im, ctx->wb, bounce, rng_out, ctx->d_counters, *aov);
    } else if (ctx->opt.counters)
        hipLaunchKernelGGL((bounce_kernel<R, MODE, true, false>), grid, dim3(256), 0, ctx->stream, sc, P, im, ctx->wb, bounce, rng_out, ctx->d_counters, AovView{});
    else
        hipLaunchKernelGGL((bounce_kernel<R, MODE, false, false>), grid, dim3(256), 0, ctx->stream, sc, P, im, ctx->wb, bounce, rng_out, ctx->d_counters, AovView{});
}

// the shade launch of one bounce, in the form and with the grid that rt_shade_launch.hpp gives it (shade_kernel: one pass, its grid from
// n0; shade_stride_kernel: any grid); aov as for launch_bounce
template <bool kSort>
static void launch_shade(rtgl_context *ctx, const rt_shade_launch::Launch &L, const SceneView &sc, const FrameParams &P, const ImageView &im, uint32_t bounce, uint4 *rng_out, const AovView *aov)
{
    using ShadeKernel = decltype(&shade_kernel<false, kSort, false>);
    static const ShadeKernel kKernels[2][2][2] = {      // [one pass][counters][first-hit planes]
        {{shade_stride_kernel<false, kSort, false>, shade_stride_kernel<false, kSort, true>}, {shade_stride_kernel<true, kSort, false>, shade_stride_kernel<true, kSort, true>}},
        {{shade_kernel<false, kSort, false>, shade_kernel<false, kSort, true>}, {shade_kernel<true, kSort, false>, shade_kernel<true, kSort, true>}}};
    if (L.one_pass) ctx->shade_pass_launches++;
    hipLaunchKernelGGL(kKernels[L.one_pass][ctx->opt.counters != 0][aov != nullptr], dim3(L.blocks), dim3(256), 0, ctx->stream, sc, P, im, ctx->wb, bounce, rng_out, ctx->d_counters, aov ? *aov : AovView{});
}

// shade_camera_kernel: bounce 0 of a lean frame, a block per 256 slots of queue 0 (the kernel makes one pass)
template <bool kSort>
static void launch_shade_camera(rtgl_context *ctx, uint32_t n0, const SceneView &sc, const FrameParams &P, const ImageView &im, uint4 *rng_out)
{
    const dim3 grid((n0 + 255u) / 256u);
    if (ctx->opt.counters) hipLaunchKernelGGL((shade_camera_kernel<true, kSort>), grid, dim3(256), 0, ctx->stream, sc, P, im, ctx->wb, rng_out, ctx->d_counters);
    else hipLaunchKernelGGL((shade_camera_kernel<false, kSort>), grid, dim3(256), 0, ctx->stream, sc, P, im, ctx->wb, rng_out, ctx->d_counters);
}

// Estimate of the rays entering `bounce`: last finished frame's count + 10 % + 2048, capped by n0.  Usually above the count, but NOT a
// bound: it survives upload_scene, and after a scene change the queue can be longer than an earlier scene's count + 10 % + 2048.  So it
// sizes the grids of kernels that grid-stride only (a low estimate costs them time, never correctness) and decides what is worth doing
// (binning); a kernel that makes one pass over its queue takes its grid from n0 (rt_shade_launch.hpp).
static uint32_t estimate_rays(const rtgl_context *ctx, uint32_t n0, uint32_t bounce)
{
    if (bounce == 0 || bounce >= ctx->est_counts.size()) return n0;
    uint64_t e = (uint64_t)ctx->est_counts[bounce] + ctx->est_counts[bounce] / 10 + 2048;
    return (uint32_t)std::min<uint64_t>(e, n0);
}

template <int R, int MODE>
static void launch_intersect(rtgl_context *ctx, const SceneView &sc, uint32_t n0, uint32_t bounce)
{
    const uint32_t chunk = (uint32_t)ctx->opt.wf_chunk;
    const uint32_t est = estimate_rays(ctx, n0, bounce);
    dim3 grid((est + 256u * R - 1) / (256u * R), (sc.n_tri_visits + chunk - 1) / chunk);
    const bool early = bounce < (uint32_t)ctx->opt.wf_early;     // wave-level edge short circuit on the coherent bounces
#define RTGL_LAUNCH_ISECT(E, P, C) hipLaunchKernelGGL((intersect_kernel<R, MODE, E, P, C>), grid, dim3(256), 0, ctx->stream, sc, ctx->wb, bounce, chunk, ctx->d_counters)
    if (early) { if (ctx->opt.counters) RTGL_LAUNCH_ISECT(true, false, true); else RTGL_LAUNCH_ISECT(true, false, false); }
    else if (ctx->opt.wf_packed) { if (ctx->opt.counters) RTGL_LAUNCH_ISECT(false, true, true); else RTGL_LAUNCH_ISECT(false, true, false); }
    else { if (ctx->opt.counters) RTGL_LAUNCH_ISECT(false, false, true); else RTGL_LAUNCH_ISECT(false, false, false); }
#undef RTGL_LAUNCH_ISECT
}

// kernel 2's intersect stage in the form options "wf_mode" and "wf_rays" name
static int launch_intersect_split(rtgl_context *ctx, const SceneView &sc, uint32_t n0, uint32_t bounce)
{
    switch (ctx->opt.wf_mode * 10 + ctx->opt.wf_rays) {
    case 1: launch_intersect<1, kScalar>(ctx, sc, n0, bounce); break;
    case 2: launch_intersect<2, kScalar>(ctx, sc, n0, bounce); break;
    case 4: launch_intersect<4, kScalar>(ctx, sc, n0, bounce); break;
    case 8: launch_intersect<8, kScalar>(ctx, sc, n0, bounce); break;
    case 11: launch_intersect<1, kLds>(ctx, sc, n0, bounce); break;
    case 12: launch_intersect<2, kLds>(ctx, sc, n0, bounce); break;
    case 14: launch_intersect<4, kLds>(ctx, sc, n0, bounce); break;
    case 18: launch_intersect<8, kLds>(ctx, sc, n0, bounce); break;
    default: return fail(ctx, RTGL_ERR_STATE, "unsupported wf_mode / wf_rays combination");
    }
    return RTGL_OK;
}

// The camera-ray bounce of one frame and the kept bits (rt_camera_keep.hpp: the rule; here: its inputs, and the buffer).  Decided once
// per frame, before ray generation is enqueued (launch_wavefront): the scan's launch of bounce 0 and the lean camera bounce both go by
// it.  cam = NULL: not a single frame of one sample.  A frame that is `cached` without `have_bits` rebuilds the bits (launch_intersect_solo).
using CameraKeep = rt_camera_keep::Decision;
static rt_camera_keep::Camera keep_camera(const FrameParams &P)
{
    rt_camera_keep::Camera c{};
    c.use_dof = P.use_dof; c.fov = P.cam_fov; c.aperture = P.cam_aperture; c.focal = P.cam_focal;
    memcpy(c.pos, P.cam_pos, sizeof c.pos); memcpy(c.forward, P.cam_forward, sizeof c.forward); memcpy(c.up, P.cam_up, sizeof c.up); memcpy(c.right, P.cam_right, sizeof c.right);
    return c;
}
static int camera_keep_decide(rtgl_context *ctx, uint32_t n0, const FrameParams *cam, CameraKeep *ck)
{
    const rt_scan_launch::Setup setup = scan_setup(ctx);
    rt_camera_keep::Frame f{};
    f.culled = rt_scan_launch::culls(setup, 0u, false); f.single = cam != nullptr; f.enabled = !getenv("RTGL_AMD_NO_CAMERA_KEEP");
    f.n0 = n0; f.words = ctx->wb.keep_words; f.scene = ctx->scene_version;
    if (cam) f.camera = keep_camera(*cam);
    const size_t need = rt_scan_launch::capacity(setup).keep_count(n0);
    f.room = ctx->keep0_capacity >= need;
    const rt_camera_keep::Key key{ctx->keep0_valid, ctx->keep0_n0, ctx->keep0_words, ctx->keep0_scene, ctx->keep0_camera};
    *ck = rt_camera_keep::decide(key, f);
    if (!ck->cached) return RTGL_OK;
    if (!ck->have_bits) ctx->keep0_valid = false;      // (valid again once packet_cull_kernel is in the stream)
    return buf_grow(ctx, ctx->d_keep0, ctx->keep0_capacity, need, need * sizeof(uint32_t));
}

// the sixteen instances of the scan, [counters][W - 1][dist]: one table for the attribute loop and for the launch
using ScanKernel = decltype(&scan_solo_kernel<false, 1, 0>);
#define RTGL_SCAN_DISTS(C, WW) {scan_solo_kernel<C, WW, 0>, scan_solo_kernel<C, WW, 1>, scan_solo_kernel<C, WW, 2>, scan_solo_kernel<C, WW, 3>}
static const ScanKernel kScanKernels[2][2][4] = {{RTGL_SCAN_DISTS(false, 1), RTGL_SCAN_DISTS(false, 2)}, {RTGL_SCAN_DISTS(true, 1), RTGL_SCAN_DISTS(true, 2)}};
#undef RTGL_SCAN_DISTS

// kernel 4: one block per CU (forced by the LDS request), persistent over the ray blocks of its triangle chunk
// ck, cam: bounce 0 only -- what camera_keep_decide said of this frame, and the frame's uniforms
static int launch_intersect_solo(rtgl_context *ctx, const SceneView &sc, uint32_t n0, uint32_t bounce, bool binned, const CameraKeep *ck, const FrameParams *cam)
{
    // 1. how this launch is cut (rt_scan_launch.hpp)
    const rt_scan_launch::Setup setup = scan_setup(ctx);
    const uint64_t items_per_wave = getenv("RTGL_AMD_ITEMS_PER_WAVE") ? (uint64_t)std::max(1, atoi(getenv("RTGL_AMD_ITEMS_PER_WAVE"))) : 3ull;      // (tuning; C2: bounce 5's launch 98 -> 89 us with three, bounces 6 and 7 +2 us each; a rank of four or eight, C4, C5: the same with two and three)
    const rt_scan_launch::Launch L = rt_scan_launch::launch(setup, items_per_wave, n0, estimate_rays(ctx, n0, bounce), bounce, binned);

    // 2. the buffers it names
#ifdef RT_SOLO_STAMPS
    if (!ctx->d_dbg_log) { RCCHK(buf_alloc(ctx, ctx->d_dbg_log, (size_t)(2 + (2u << 22)) * 4)); HIPCHK(ctx, hipMemsetAsync(ctx->d_dbg_log, 0, 2048 * 8 + 16 * 64 * 2 * 16 * 8, ctx->stream)); }
#endif
    MfView mf{ctx->d_mf_groups, ctx->n_mf_groups, ctx->mf_group_quads, ctx->n_mf_groups * ctx->mf_group_quads, ctx->d_mf_A, ctx->d_dbg_log, ctx->d_mf_cull, ctx->d_edges_s, ctx->d_planes_s, ctx->d_mf_order};
    if (!ctx->solo_attr_set) {
        // allow the whole LDS of a CU (160 KB) minus the kernel's static share as dynamic shared memory.  The attribute belongs to the
        // (function, device) pair, so it is raised once per context -- a context is bound to one device -- not once per process.
        for (const auto &by_w : kScanKernels) for (const auto &by_dist : by_w) for (const ScanKernel k : by_dist) {
            const void *fn = reinterpret_cast<const void *>(k);
            hipFuncAttributes fattr;
            HIPCHK(ctx, hipFuncGetAttributes(&fattr, fn));
            HIPCHK(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024 - fattr.sharedSizeBytes)));
        }
        ctx->solo_attr_set = true;
    }
    float ro_add = 0.0f, sigma_add = 0.0f; bool have_bits = false;
    const bool cached = L.cull && bounce == 0 && ck && cam && ck->cached;
    if (L.cull) {
        // camera-ray bounce of a single frame: the bits of an earlier frame of the same camera, image and scene, if there are any
        if (cached) { ctx->wb.keep = ctx->d_keep0; have_bits = ck->have_bits; ro_add = ck->ro_add; sigma_add = ck->sigma_add; }
        else ctx->wb.keep = ctx->d_keep;
        if (L.dist == 2) {
            RCCHK(buf_grow(ctx, ctx->d_plan, ctx->plan_capacity, L.plan_need, L.plan_need));
            ctx->wb.plan_prefix = reinterpret_cast<uint32_t *>(ctx->d_plan); ctx->wb.plan_stride = L.stride;
            ctx->wb.plan_total = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ctx->d_plan) + L.plan_off_tot);
            ctx->wb.plan_base = reinterpret_cast<unsigned long long *>(reinterpret_cast<uint8_t *>(ctx->d_plan) + L.plan_off_base);
        }
        if (L.dist == 1) {
            RCCHK(buf_grow(ctx, ctx->d_items, ctx->items_capacity, L.items_need, L.items_need));
            ctx->wb.item_counts = reinterpret_cast<uint32_t *>(ctx->d_items);
            ctx->wb.items = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ctx->d_items) + L.items_head);
            ctx->wb.items_stride = L.stride;
        }
    }

    // 3. the launches
    if (L.cull) {
        // (a binned queue is always culled here, and never from kept bits: bounce >= 1.  Under RTGL_AMD_SORT_MOVE = 1 this launch is what
        // moves its rays out of the staging queue)
        if (!have_bits) {
            hipLaunchKernelGGL(packet_cull_kernel, dim3(L.cull_blocks), dim3(256), 0, ctx->stream, ctx->wb, ctx->d_mf_cull, setup.real_quads * (uint32_t)kMfQuadTiles, bounce, ro_add, sigma_add,
                               ctx->d_mf_cull_node, ctx->d_mf_cull_node ? ctx->cull_node_shift : 0u, (uint32_t)(binned && ctx->opt.sort_move == 1));
            if (cached) {
                // the camera's bits are in the stream: from here on they serve the frames of this camera, image and scene (a frame that
                // fails drops them again: render_batch)
                HIPCHK(ctx, hipGetLastError());
                ctx->keep0_valid = true; ctx->keep0_n0 = n0; ctx->keep0_words = ctx->wb.keep_words; ctx->keep0_scene = ctx->scene_version; ctx->keep0_camera = keep_camera(*cam);
            }
        }
        if (L.dist == 2) {
            hipLaunchKernelGGL(ctx->opt.counters ? scan_plan_kernel<true> : scan_plan_kernel<false>, dim3(L.chunks), dim3(256), 0, ctx->stream, ctx->wb, bounce, L.chunk_quads, setup.real_quads, ctx->d_counters);
            hipLaunchKernelGGL(scan_plan_base_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->wb, L.chunks);
        }
        if (L.dist == 1) {
            HIPCHK(ctx, hipMemsetAsync(ctx->wb.item_counts, 0, (size_t)L.chunks * sizeof(uint32_t), ctx->stream));
            hipLaunchKernelGGL(ctx->opt.counters ? cull_items_kernel<true> : cull_items_kernel<false>, dim3(L.items_grid_x, L.items_grid_y), dim3(256), 0, ctx->stream, ctx->wb, bounce, L.chunk_quads, setup.real_quads, ctx->d_counters);
        }
    }
    // (testing the survivors of small launches in place instead of launching the narrow phase was measured: never faster --
    // rank of eight 0.73 -> 0.76-0.85 ms)
    // "narrow_fused": every scan wave tests the records of its own region when it has run out of items (rt_scan.hpp, tail drain), and
    // the narrow phase is not launched.  (Not the experiment above, which ran the tests inside flush(), in the middle of the item loop.)
    // C2 +2.2 %, C5 +1.2 %, C4 +1.5 %: the scan launches grow by 109 us per C2 frame, the narrow phase's 152 us go (DESIGN.md 9 item 2;
    // profiles/narrow_fused_c2/ab.txt).  The stamps builds keep the separate launch: their per-bounce bookkeeping lives in narrow_phase_kernel.
#ifdef RT_SOLO_STAMPS
    const int fused = 0;
#else
    const int fused = ctx->opt.narrow_fused;
#endif
    hipLaunchKernelGGL(kScanKernels[ctx->opt.counters != 0][L.W - 1][L.dist], dim3(L.blocks), dim3(256 * L.W), L.lds, ctx->stream, sc, ctx->wb, mf, bounce, L.chunk_quads, L.chunks, ctx->d_counters, ctx->opt.debug_skip_exact, L.cull, fused);
    HIPCHK(ctx, hipGetLastError());
    if (!fused) hipLaunchKernelGGL(narrow_phase_kernel, dim3(L.blocks * L.waves, kNarrowSplit), dim3(256), 0, ctx->stream, sc, ctx->wb, mf, bounce, L.blocks * L.waves);
    return RTGL_OK;
}

// frames.size() > 1: a batch -- every frame's camera rays are generated into its own stretch of queue 0 (n0_frame slots), everything
// behind that sees ONE frame of n0 = B x n0_frame rays, and resolve_batch_kernel applies the frames' results to the image in order
// masked != NULL: a masked frame of adaptive sampling (rt_adaptive.hpp) -- one frame whose queue 0 holds the n0_frame / 64 blocks of that
// list.  The keep cache's key knows n0 and the camera but not the mask, so such a frame stays out of it: it runs as `cam == NULL` does.
static int launch_wavefront(rtgl_context *ctx, const SceneView &sc, const std::vector<FrameParams> &frames, const ImageView &im, uint32_t n0_frame, uint4 *rng_out,
                            const AovView *aov, const uint32_t *masked = nullptr)
{
    const FrameParams &P = frames[0];
    const uint32_t B = (uint32_t)frames.size(), n0 = n0_frame * B;
    const dim3 gen_grid((n0_frame + 255) / 256);
    // pick up the ray counts of the most recent finished frame (never blocks)
    if (ctx->counts_pending && hipEventQuery(ctx->counts_ev) == hipSuccess) {
        ctx->counts_pending = false;
        if (ctx->counts_n0 == n0) ctx->est_counts.assign(ctx->h_counts, ctx->h_counts + ctx->counts_len);
        else ctx->est_counts.clear();
        // the fullest candidate region of that frame: grow before the NEXT frame is enqueued (ensure_wave_buffers), never shrink
        const uint32_t peak = ctx->h_counts[ctx->counts_capacity];
        if (!ctx->cand_fixed && peak > ctx->cand_region_pairs) ctx->cand_region_target = (uint32_t)std::min<uint64_t>((uint64_t)peak + peak / 4, 0xFFFFFFF0u);
    }
    // the camera-ray bounce: from kept bits?  And then in its lean form (option "camera_lean"): a single frame of one sample, no first-hit planes
    CameraKeep ck{};
    const FrameParams *const cam = (B == 1 && P.samples == 1u && !masked) ? &P : nullptr;
    if (ctx->opt.kernel == RTGL_KERNEL_WAVEFRONT_MFMA_SOLO && sc.n_tri_visits > 0 && P.max_bounce > 0) RCCHK(camera_keep_decide(ctx, n0, cam, &ck));
    const bool lean = rt_camera_keep::lean(ck, ctx->opt.camera_lean, aov != nullptr);
    if (lean) ctx->camera_lean_frames++;
    for (uint32_t s = 0; s < P.samples; ++s) {
        const uint32_t n_counts = ctx->counts_capacity + 1u <= 256u ? ctx->counts_capacity + 1u : 0u;      // cleared by generate_rays_kernel's first block
        if (!n_counts) HIPCHK(ctx, hipMemsetAsync(ctx->d_counts, 0, counts_bytes(ctx->counts_capacity), ctx->stream));
        // the scan launches' work counters (rt_scan.hpp): cleared by the first threads of generate_rays_kernel where there are enough of them
        uint32_t n_sched = 0u;
        if (ctx->opt.kernel == RTGL_KERNEL_WAVEFRONT_MFMA_SOLO && ctx->d_sched && rt_scan_launch::uses_claim_counters(rt_scan_launch::mesh_dist(scan_setup(ctx)))) {      // (the mesh-level choice, not a launch's dist)
            const size_t words = (size_t)(P.max_bounce + 2) * ctx->wb.sched_stride;
            if (words <= (size_t)gen_grid.x * 256u && !getenv("RTGL_AMD_SCHED_FILL")) n_sched = (uint32_t)words;      // (the variable: measurement of the fill launch this replaces)
            else HIPCHK(ctx, hipMemsetAsync(ctx->d_sched, 0, words * sizeof(uint32_t), ctx->stream));
        }
        if (masked)
            hipLaunchKernelGGL(generate_rays_masked_kernel, gen_grid, dim3(256), 0, ctx->stream, P, im, ctx->wb, masked, n0_frame, ctx->opt.counters ? ctx->d_counters : (Counters *)nullptr, n_counts, n_sched);
        else for (uint32_t f = 0; f < B; ++f)
            hipLaunchKernelGGL(generate_rays_kernel, gen_grid, dim3(256), 0, ctx->stream, frames[f], im, ctx->wb, s, n0_frame,
                               ctx->opt.counters ? ctx->d_counters : (Counters *)nullptr, f == 0 ? n_counts : 0u, f * n0_frame, B > 1 ? f << 28 : 0u, f == 0 ? n0 : 0u, f == 0 ? n_sched : 0u,
                               lean ? 1u : 0u);
        bool binned = false;                                 // the queue of the bounce about to be launched was binned
        for (uint32_t b = 0; b < P.max_bounce; ++b) {
            const int key = ctx->opt.wf_mode * 10 + ctx->opt.wf_rays;
            const AovView *aov_b = (s == 0u && b == 0u) ? aov : nullptr;      // the first-hit planes: the camera rays of sample 0
            if (ctx->opt.kernel == RTGL_KERNEL_WAVEFRONT_SPLIT || ctx->opt.kernel == RTGL_KERNEL_WAVEFRONT_MFMA_SOLO) {
                if (sc.n_tri_visits > 0 && ctx->opt.kernel == RTGL_KERNEL_WAVEFRONT_MFMA_SOLO) {
                    kev_mark(ctx);
                    { const int rc = launch_intersect_solo(ctx, sc, n0, b, binned, b == 0u ? &ck : nullptr, cam); if (rc) return rc; }
                    kev_mark(ctx);
                } else if (sc.n_tri_visits > 0) {
                    kev_mark(ctx);
                    RCCHK(launch_intersect_split(ctx, sc, n0, b));
                    kev_mark(ctx);
                }
                // ray binning: the queue of the next bounce in (direction bin, origin cell) order, where it is long enough to pay for
                // the three small launches and the extra pass over its rays
                const uint32_t est_next = estimate_rays(ctx, n0, b + 1u);
                const bool bin_next = ctx->opt.kernel == RTGL_KERNEL_WAVEFRONT_MFMA_SOLO && ctx->opt.cull == 3 && sc.n_tri_visits > 0 && b + 1u < P.max_bounce
                                      && est_next >= (uint32_t)ctx->opt.sort_min_rays;
                const rt_shade_launch::Launch shade = rt_shade_launch::launch(ctx->opt.shade_pass, n0, estimate_rays(ctx, n0, b), bin_next);
                if (bin_next) {
                    // two sets of bin counters take turns: the move (sort_place_kernel or sort_scatter_kernel) zeroes the one the next binned bounce will count in
                    const rt_bin_plan::Plan plan = {ctx->wb.sort_ob, ctx->wb.sort_cells.db, ctx->wb.sort_bits, ctx->wb.sort_cells.T, false};
                    const size_t bins = rt_bin_plan::bins(plan), set_words = rt_bin_plan::set_words(plan);
                    if (!ctx->sort_sets_clean || ctx->sort_set_bits != ctx->wb.sort_bits) {
                        HIPCHK(ctx, hipMemsetAsync(ctx->d_sort_hist, 0, rt_bin_plan::hist_words(plan) * sizeof(uint32_t), ctx->stream));
                        ctx->sort_set = 0; ctx->sort_set_bits = ctx->wb.sort_bits;
                    }
                    ctx->sort_sets_clean = false;              // (true again once this bounce's launches are in the stream)
                    if (getenv("RTGL_AMD_HIST_FILL")) HIPCHK(ctx, hipMemsetAsync(ctx->d_sort_hist + (size_t)ctx->sort_set * set_words, 0, bins * sizeof(uint32_t), ctx->stream));      // (measurement: the fill launch per bounce that the turns replace)
                    ctx->wb.sort_hist = ctx->d_sort_hist + (size_t)ctx->sort_set * set_words;
                    ctx->wb.sort_hist_other = ctx->d_sort_hist + (size_t)(ctx->sort_set ^ 1) * set_words;
                    if (lean && b == 0u) launch_shade_camera<true>(ctx, n0, sc, P, im, rng_out);
                    else launch_shade<true>(ctx, shade, sc, P, im, b, rng_out, aov_b);
                    hipLaunchKernelGGL(sort_sums_kernel, dim3(rt_bin_plan::sums_grid(plan)), dim3(256), 0, ctx->stream, ctx->wb);
                    hipLaunchKernelGGL(sort_prefix_kernel, dim3(rt_bin_plan::sums_grid(plan)), dim3(256), 0, ctx->stream, ctx->wb);
                    // (the move: the rays' staging slots in key order, gathered by the next bounce's packet_cull_kernel; or, option 0, the rays themselves)
                    if (ctx->opt.sort_move == 1) hipLaunchKernelGGL(sort_place_kernel, dim3(std::max(1u, std::min((est_next + 255u) / 256u, 16384u))), dim3(256), 0, ctx->stream, ctx->wb, b + 1u);
                    else hipLaunchKernelGGL(sort_scatter_kernel, dim3(std::max(1u, std::min((est_next + 255u) / 256u, 16384u))), dim3(256), 0, ctx->stream, ctx->wb, b + 1u);
                    HIPCHK(ctx, hipGetLastError());
                    ctx->sort_set ^= 1; ctx->sort_sets_clean = true;
                } else if (lean && b == 0u) launch_shade_camera<false>(ctx, n0, sc, P, im, rng_out);
                else launch_shade<false>(ctx, shade, sc, P, im, b, rng_out, aov_b);
                binned = bin_next;
                continue;
            }
            kev_mark(ctx);
            switch (key) {
            case 1: launch_bounce<1, kScalar>(ctx, sc, P, im, n0, b, rng_out, aov_b); break;
            case 2: launch_bounce<2, kScalar>(ctx, sc, P, im, n0, b, rng_out, aov_b); break;
            case 4: launch_bounce<4, kScalar>(ctx, sc, P, im, n0, b, rng_out, aov_b); break;
            case 11: launch_bounce<1, kLds>(ctx, sc, P, im, n0, b, rng_out, aov_b); break;
            case 12: launch_bounce<2, kLds>(ctx, sc, P, im, n0, b, rng_out, aov_b); break;
            case 14: launch_bounce<4, kLds>(ctx, sc, P, im, n0, b, rng_out, aov_b); break;
            default: return fail(ctx, RTGL_ERR_STATE, "unsupported wf_mode / wf_rays combination");
            }
            kev_mark(ctx);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    if (P.samples > 1u) {
        hipLaunchKernelGGL(resolve_kernel, gen_grid, dim3(256), 0, ctx->stream, P, im, ctx->wb);
        HIPCHK(ctx, hipGetLastError());
    }
    if (B > 1) {
        BatchInfo bi{};
        bi.n = B;
        for (uint32_t f = 0; f < B; ++f) { bi.frames[f] = frames[f].frames; bi.reset[f] = frames[f].reset_flag; }
        hipLaunchKernelGGL(resolve_batch_kernel, gen_grid, dim3(256), 0, ctx->stream, im, ctx->wb, bi);
        HIPCHK(ctx, hipGetLastError());
    }
    if (!ctx->counts_pending) {      // feed the next frames' grid sizes; skipped while an earlier copy is in flight
        ctx->counts_len = P.max_bounce + 1; ctx->counts_n0 = n0;
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_counts, ctx->d_counts, counts_bytes(ctx->counts_capacity), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipEventRecord(ctx->counts_ev, ctx->stream));
        ctx->counts_pending = true;
    }
    return RTGL_OK;
}

extern "C" int rtgl_set_frame_params(rtgl_context *ctx, const rtgl_frame_params *p)
{
    ENTER_NOFLUSH(ctx);
    FANOUT(ctx, rtgl_set_frame_params(part, p));
    if (!p) return fail(ctx, RTGL_ERR_INVALID, "params is NULL");
    static_assert(sizeof(FrameParams) == sizeof(rtgl_frame_params), "FrameParams mirrors rtgl_frame_params");
    memcpy(&ctx->params, p, sizeof(FrameParams));
    ctx->have_params = true;
    return RTGL_OK;
}

static int render_batch(rtgl_context *ctx, const std::vector<FrameParams> &batch);

// what the frames of a batch must share: everything the kernels behind ray generation read from the uniforms
static bool batch_compatible(const FrameParams &a, const FrameParams &b)
{
    return a.samples == b.samples && a.max_bounce == b.max_bounce && a.use_envmap == b.use_envmap && memcmp(a.background, b.background, sizeof a.background) == 0;
}

static int flush_pending(rtgl_context *ctx)
{
    if (ctx->pending.empty()) return RTGL_OK;
    std::vector<FrameParams> batch;
    batch.swap(ctx->pending);
    return render_batch(ctx, batch);
}

extern "C" int rtgl_render_frame(rtgl_context *ctx)
{
    ENTER_NOFLUSH(ctx);
    if (!ctx->workers.empty()) {                         // every part's frame is submitted by its own thread; this one waits for all of them
        ctx->gathered = false;
        for (auto &w : ctx->workers) { { std::lock_guard<std::mutex> lk(w->m); w->state = PartWorker::kJob; } w->cv.notify_all(); }
        int first = RTGL_OK; const rtgl_context *bad = nullptr;
        for (auto &w : ctx->workers) {
            std::unique_lock<std::mutex> lk(w->m);
            w->cv.wait(lk, [&w] { return w->state == PartWorker::kDone; });
            w->state = PartWorker::kIdle;
            if (w->rc && !first) { first = w->rc; bad = w->part; }
        }
        return first ? fail(ctx, first, std::string("device ") + std::to_string(bad->device) + ": " + bad->error) : RTGL_OK;
    }
    FANOUT(ctx, rtgl_render_frame(part));
    if (!ctx->have_params) return fail(ctx, RTGL_ERR_STATE, "rtgl_set_frame_params has not been called");
    if (ctx->params.samples == 0) return fail(ctx, RTGL_ERR_INVALID, "u_samples == 0 divides by zero in the reference; refused");
    ctx->ad.active = false;                              // (adaptive sampling: an ordinary frame ends the session; one refused above does not)
    // frame batching: hold the frame back until the batch is full.  Only what the batched pipeline covers: one sample per frame, the
    // per-bounce pipeline (a scene with triangles), no per-frame read-outs (counters, RNG states)
    const bool batchable = ctx->opt.frame_batch > 1 && ctx->params.samples == 1 && ctx->params.max_bounce > 0 && !ctx->opt.counters && !ctx->opt.rng_state
                           && !ctx->opt.kernel_timing && !ctx->opt.aov && (ctx->n_tri_visits > 0 || ctx->tris_dirty || ctx->kernel_explicit) && ctx->opt.kernel != RTGL_KERNEL_MEGA;
    if (!ctx->pending.empty() && (!batchable || !batch_compatible(ctx->pending.front(), ctx->params))) { const int rc = flush_pending(ctx); if (rc) return rc; }
    if (batchable) {
        ctx->pending.push_back(ctx->params);
        return (int)ctx->pending.size() >= ctx->opt.frame_batch ? flush_pending(ctx) : RTGL_OK;
    }
    return render_batch(ctx, std::vector<FrameParams>(1, ctx->params));
}

// the scene as the kernels see it
static SceneView scene_view(const rtgl_context *ctx)
{
    SceneView sc{};
    sc.spheres = ctx->d_spheres; sc.n_spheres = ctx->n_spheres;
    sc.sphere_visits = ctx->d_sphere_visits; sc.n_sphere_visits = ctx->n_sphere_visits;
    sc.materials = ctx->d_materials; sc.n_materials = ctx->n_materials;
    sc.tri_edges = ctx->d_edges; sc.tri_planes = ctx->d_planes; sc.n_tri_visits = ctx->n_tri_visits;
    sc.env = ctx->d_env; sc.env_w = ctx->env_w; sc.env_h = ctx->env_h; sc.env_c = ctx->env_c; sc.env_faces = ctx->env_faces;
    return sc;
}

// the ids plane's mesh and triangle of every triangle visit, uploaded once per rebuild of the triangles and only while the plane is on
static int upload_visit_ids(rtgl_context *ctx)
{
    if (!(ctx->opt.aov & RTGL_AOV_IDS) || !ctx->visit_ids_dirty) return RTGL_OK;
    const size_t bytes = ctx->h_visit_tri.size() * sizeof(uint32_t);
    RCCHK(realloc_upload(ctx, ctx->d_visit_mesh, ctx->h_visit_mesh.data(), bytes));
    RCCHK(realloc_upload(ctx, ctx->d_visit_tri, ctx->h_visit_tri.data(), bytes));
    ctx->visit_ids_dirty = false;
    return RTGL_OK;
}

// one frame, or the frames of a batch in one set of launches
static int render_batch(rtgl_context *ctx, const std::vector<FrameParams> &batch)
{
    const uint32_t B = (uint32_t)batch.size();
    for (const FrameParams &f : batch) {                 // rtgl_error_estimate: a reset frame starts a new accumulation; the latest frame's `frames`
        rt_error_plan::rendered_frame(ctx->err, f.frames, f.reset_flag != 0);
    }
    if (ctx->visits_dirty) { int rc = rebuild_sphere_visits(ctx); if (rc) return rc; }
    if (ctx->tris_dirty) { int rc = rebuild_triangles(ctx); if (rc) return rc; }
    if (ctx->opt.rng_state) RCCHK(buf_ensure(ctx, ctx->d_rng, local_px(ctx) * sizeof(uint4)));
    RCCHK(upload_visit_ids(ctx));

    const SceneView sc = scene_view(ctx);
    std::vector<FrameParams> frames(batch);
    for (FrameParams &f : frames) if (!ctx->d_env) f.use_envmap = 0;   // src/renderer.cpp:104-110: no cube map => u_use_envmap = false
    const FrameParams &P = frames[0];
    ImageView im{};
    im.pixels = ctx->d_image; im.width = ctx->width; im.height = ctx->height;
    im.disp_w = ctx->width / 8 * 8; im.disp_h = ctx->height / 8 * 8;
    im.local_rows = ctx->local_rows; im.rank = ctx->rank; im.world = ctx->world; im.strip_rows = ctx->strip_rows;

    if (ctx->opt.counters) HIPCHK(ctx, hipMemsetAsync(ctx->d_counters, 0, sizeof(Counters), ctx->stream));
    // rows of the dispatch footprint held locally: a prefix of the local rows (strips are 8-row aligned)
    int local_disp_rows = 0;
    for (int lr = 0; lr < ctx->local_rows; ++lr) if (rtgl_local_row_to_global(ctx, lr) < im.disp_h) local_disp_rows = lr + 1;
    const uint32_t n0_frame = (uint32_t)im.disp_w * (uint32_t)local_disp_rows;
    if ((uint64_t)n0_frame * B > 0xFFFFFFF0ull || local_px(ctx) > (size_t)kBatchPixelMask) return fail(ctx, RTGL_ERR_INVALID, "frame_batch: the batch does not fit 32-bit ray slots");
    const uint32_t n0 = n0_frame * B;            // rays entering bounce 0: all frames of the batch
    uint4 *rng_out = ctx->opt.rng_state ? ctx->d_rng : nullptr;
    // first-hit planes: frames are rendered one by one while they are on (B == 1); the running mean restarts with a reset frame
    AovView aov{};
    if (ctx->opt.aov) {
        ctx->aov_n = (P.reset_flag || ctx->aov_restart) ? 1u : ctx->aov_n + 1u;
        ctx->aov_restart = false;
        aov.albedo = ctx->d_aov[0]; aov.normal = ctx->d_aov[1]; aov.position = ctx->d_aov[2]; aov.ids = ctx->d_aov_ids;
        aov.visit_mesh = ctx->d_visit_mesh; aov.visit_tri = ctx->d_visit_tri; aov.n = ctx->aov_n;
    }
    // a scene without triangles has no scan to split off: one megakernel launch per frame beats the per-bounce pipeline
    // (C1, 256x256 spheres: 1460 vs 1025 Mpaths/s) unless the caller asked for a specific variant
    const int kernel = (ctx->n_tri_visits == 0 && !ctx->kernel_explicit) ? (int)RTGL_KERNEL_MEGA : ctx->opt.kernel;
    const bool use_wavefront = kernel != RTGL_KERNEL_MEGA && P.max_bounce > 0;
    ctx->kernel_in_use = use_wavefront ? kernel : (int)RTGL_KERNEL_MEGA;
    if (B > 1 && !(use_wavefront && n0 > 0)) {          // (nothing to batch: a scene that lost its triangles meanwhile, an empty tile) one frame at a time
        for (const FrameParams &f : batch) { const int rc = render_batch(ctx, std::vector<FrameParams>(1, f)); if (rc) return rc; }
        return RTGL_OK;
    }
    if (use_wavefront && n0 > 0) { int rc = ensure_wave_buffers(ctx, n0, P.max_bounce, P.samples > 1); if (rc) return rc; }
    ctx->wb.batch_rad = nullptr; ctx->wb.batch_px = 0;
    if (B > 1) {
        const size_t need = local_px(ctx) * B;
        RCCHK(buf_grow(ctx, ctx->d_batch_rad, ctx->batch_capacity, need, need * sizeof(float4)));
        ctx->wb.batch_rad = ctx->d_batch_rad; ctx->wb.batch_px = (uint32_t)local_px(ctx);
    }
    ctx->last_batch_frames = B;
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    // option kernel_timing = N: every N-th frame since the last reset carries the event pairs (each pair costs ~3 us of gap)
    ctx->timing_this_frame = ctx->opt.kernel_timing > 0 && (ctx->timing_frame_counter++ % (uint32_t)ctx->opt.kernel_timing) == 0u;
    if (ctx->timing_this_frame) {
        if (ctx->kev_frame_start.size() >= 4096) { ctx->kev_used = 0; ctx->kev_frame_start.clear(); }   // bounded history
        ctx->kev_frame_start.push_back(ctx->kev_used);
        kev_mark(ctx);                                   // frame begin
    }
    if (n0 > 0 && !use_wavefront) {
        dim3 grid((im.disp_w + 31) / 32, (local_disp_rows + 7) / 8);
        kev_mark(ctx);
        if (ctx->opt.aov) {
            if (ctx->opt.counters) hipLaunchKernelGGL((pathtrace_mega_kernel<true, true>), grid, dim3(256), 0, ctx->stream, sc, P, im, rng_out, ctx->d_counters, aov);
            else hipLaunchKernelGGL((pathtrace_mega_kernel<false, true>), grid, dim3(256), 0, ctx->stream, sc, P, im, rng_out, ctx->d_counters, aov);
        } else if (ctx->opt.counters)
            hipLaunchKernelGGL((pathtrace_mega_kernel<true, false>), grid, dim3(256), 0, ctx->stream, sc, P, im, rng_out, ctx->d_counters, AovView{});
        else
            hipLaunchKernelGGL((pathtrace_mega_kernel<false, false>), grid, dim3(256), 0, ctx->stream, sc, P, im, rng_out, ctx->d_counters, AovView{});
        kev_mark(ctx);
        HIPCHK(ctx, hipGetLastError());
    } else if (n0 > 0) {
        int rc = launch_wavefront(ctx, sc, frames, im, n0_frame, rng_out, ctx->opt.aov ? &aov : nullptr);
        if (rc) { ctx->keep0_valid = false; return rc; }      // (a frame that failed half way vouches for nothing it left behind)
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    kev_mark(ctx);                                       // frame end
    ctx->timed = true;
    return RTGL_OK;
}

extern "C" int rtgl_synchronize(rtgl_context *ctx)
{
    ENTER(ctx);
    for (rtgl_context *part : ctx->parts) { const int rc = rtgl_synchronize(part); if (rc) return fail(ctx, rc, part->error); }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RTGL_OK;
}

extern "C" int rtgl_last_frame_ms(rtgl_context *ctx, float *ms)
{
    ENTER(ctx);
    if (!ctx->parts.empty()) {
        if (!ms) return fail(ctx, RTGL_ERR_INVALID, "ms is NULL");
        *ms = 0.0f;
        for (rtgl_context *part : ctx->parts) { float m = 0.0f; const int rc = rtgl_last_frame_ms(part, &m); if (rc) return fail(ctx, rc, part->error); *ms = std::max(*ms, m); }
        return RTGL_OK;
    }
    if (!ms || !ctx->timed) return fail(ctx, RTGL_ERR_STATE, "no frame has been rendered");
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    *ms /= (float)std::max(ctx->last_batch_frames, 1u);          // a batch of frames was timed as one
    return RTGL_OK;
}

// sums the event pairs of frames [first, last) of the recorded history
static int sum_timing(rtgl_context *ctx, size_t first, size_t last, rtgl_frame_timing *out)
{
    memset(out, 0, sizeof *out);
    for (size_t f = first; f < last; ++f) {
        const uint32_t b = ctx->kev_frame_start[f], e = (f + 1 < ctx->kev_frame_start.size()) ? ctx->kev_frame_start[f + 1] : ctx->kev_used;
        if (e < b + 2) continue;
        float ms = 0.0f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->kev[b], ctx->kev[e - 1]));
        out->frame_ms += ms;
        for (uint32_t i = b + 1; i + 1 < e - 1; i += 2) {
            HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->kev[i], ctx->kev[i + 1]));
            out->intersect_ms += ms; out->intersect_launches++;
        }
    }
    return RTGL_OK;
}

extern "C" int rtgl_last_frame_timing(rtgl_context *ctx, rtgl_frame_timing *out)
{
    ENTER(ctx);
    if (!ctx->parts.empty()) { const int rc = rtgl_last_frame_timing(ctx->parts[0], out); return rc ? fail(ctx, rc, ctx->parts[0]->error) : RTGL_OK; }   // device 0's share
    if (!out || !ctx->timed) return fail(ctx, RTGL_ERR_STATE, "no frame has been rendered");
    if (!ctx->opt.kernel_timing || ctx->kev_frame_start.empty()) return fail(ctx, RTGL_ERR_STATE, "option kernel_timing was not enabled before rendering");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return sum_timing(ctx, ctx->kev_frame_start.size() - 1, ctx->kev_frame_start.size(), out);
}

extern "C" int rtgl_accumulated_timing(rtgl_context *ctx, rtgl_frame_timing *out, uint32_t *frames_out)
{
    ENTER(ctx);
    if (!ctx->parts.empty()) { const int rc = rtgl_accumulated_timing(ctx->parts[0], out, frames_out); return rc ? fail(ctx, rc, ctx->parts[0]->error) : RTGL_OK; }
    if (!out) return fail(ctx, RTGL_ERR_INVALID, "out is NULL");
    if (!ctx->opt.kernel_timing) return fail(ctx, RTGL_ERR_STATE, "option kernel_timing is not enabled");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (frames_out) *frames_out = (uint32_t)ctx->kev_frame_start.size();
    return sum_timing(ctx, 0, ctx->kev_frame_start.size(), out);
}

extern "C" int rtgl_timing_reset(rtgl_context *ctx)
{
    ENTER(ctx);
    FANOUT(ctx, rtgl_timing_reset(part));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->kev_used = 0; ctx->kev_frame_start.clear(); ctx->timing_frame_counter = 0;
    return RTGL_OK;
}

extern "C" int rtgl_read_image_f32(rtgl_context *ctx, float *rgba)
{
    ENTER(ctx);
    if (!rgba) return fail(ctx, RTGL_ERR_INVALID, "rgba is NULL");
    if (!ctx->parts.empty()) { const int rc = multi_gather(ctx); if (rc) return rc; }
    return read_rows(ctx, rgba, ctx->d_image, 16);
}

extern "C" int rtgl_write_image_f32(rtgl_context *ctx, const float *rgba)
{
    ENTER(ctx);
    if (!rgba) return fail(ctx, RTGL_ERR_INVALID, "rgba is NULL");
    rt_error_plan::drop(ctx->err);                      // (rtgl_error_estimate: another image, the snapshot is dropped)
    ctx->ad.active = false;                             // (adaptive sampling: ... and the session ends)
    if (!ctx->parts.empty()) {                          // scatter the rows to their owners
        ctx->gathered = false;
        std::vector<float> local;
        for (rtgl_context *part : ctx->parts) {
            local.resize(local_px(part) * 4);
            for (int lr = 0; lr < part->local_rows; ++lr)
                memcpy(local.data() + (size_t)lr * ctx->width * 4, rgba + (size_t)rtgl_local_row_to_global(part, lr) * ctx->width * 4, (size_t)ctx->width * 16);
            const int rc = rtgl_write_image_f32(part, local.data());
            if (rc) return fail(ctx, rc, part->error);
        }
        return RTGL_OK;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_image, rgba, (size_t)ctx->local_rows * ctx->width * 16, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RTGL_OK;
}

extern "C" int rtgl_clear_image(rtgl_context *ctx)
{
    ENTER(ctx);
    FANOUT(ctx, rtgl_clear_image(part));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_image, 0, (size_t)ctx->local_rows * ctx->width * 16, ctx->stream));
    ctx->aov_restart = true;                              // the first-hit planes' mean restarts with the next frame (their contents stay)
    rt_error_plan::drop(ctx->err);                        // (rtgl_error_estimate: the snapshot is dropped)
    ctx->ad.active = false;                               // (adaptive sampling: the session ends)
    return RTGL_OK;
}

extern "C" int rtgl_read_image_u8(rtgl_context *ctx, uint8_t *rgba, int flip)
{
    ENTER(ctx);
    if (!rgba) return fail(ctx, RTGL_ERR_INVALID, "rgba is NULL");
    if (!ctx->parts.empty()) { const int rc = multi_gather(ctx); if (rc) return rc; }
    size_t n = (size_t)ctx->local_rows * ctx->width;
    if (n == 0) return RTGL_OK;
    RCCHK(buf_ensure(ctx, ctx->d_u8, n * 4));
    hipLaunchKernelGGL(image_to_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       ctx->d_image, ctx->d_u8, ctx->width, ctx->local_rows, flip);
    HIPCHK(ctx, hipGetLastError());
    return read_rows(ctx, rgba, ctx->d_u8, 4);
}

extern "C" int rtgl_local_rows(const rtgl_context *ctx) { return ctx ? ctx->local_rows : RTGL_ERR_INVALID; }

extern "C" int rtgl_local_row_to_global(const rtgl_context *ctx, int lr)
{
    if (!ctx || lr < 0 || lr >= ctx->local_rows) return RTGL_ERR_INVALID;
    if (ctx->world == 1) return lr;
    int ls = lr / ctx->strip_rows, within = lr - ls * ctx->strip_rows;
    return (ls * ctx->world + ctx->rank) * ctx->strip_rows + within;
}

extern "C" void *rtgl_device_image(rtgl_context *ctx)
{
    if (!ctx) return nullptr;
    if (!ctx->pending.empty()) {                         // frames a batching context still holds back: a failed submission is an error, not a stale image
        if (hipSetDevice(ctx->device) != hipSuccess) { ctx->error = "rtgl_device_image: hipSetDevice failed"; return nullptr; }
        if (flush_pending(ctx) != RTGL_OK) return nullptr;      // (ctx->error holds the reason)
    }
    return (void *)ctx->d_image;
}

extern "C" int rtgl_bind_device_image(rtgl_context *ctx, void *dptr)
{
    ENTER(ctx);
    if (!ctx->parts.empty()) return fail(ctx, RTGL_ERR_STATE, "a multi-device context renders into its own per-device tile buffers");
    ctx->d_image = dptr ? (float4 *)dptr : ctx->d_image_own;
    rt_error_plan::drop(ctx->err);                        // (rtgl_error_estimate: another image, the snapshot is dropped)
    ctx->ad.active = false;                               // (adaptive sampling: ... and the session ends)
    return RTGL_OK;
}

extern "C" int rtgl_set_stream(rtgl_context *ctx, void *hip_stream)
{
    ENTER(ctx);
    if (!ctx->parts.empty()) return fail(ctx, RTGL_ERR_STATE, "a multi-device context owns one stream per device");
    const hipStream_t want = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    if (want != ctx->own_stream && other_stream_in_use(ctx, ctx->device, want) && !concurrent_pipelines_allowed())
        return fail(ctx, RTGL_ERR_STATE, "rtgl_set_stream: another context of this process renders on a different stream of this device; two path-tracing pipelines "
                                         "running concurrently on one device have produced wrong frames (DESIGN.md 5.2).  Bind the SAME stream to all of them, or set "
                                         "RTGL_AMD_ALLOW_CONCURRENT_PIPELINES=1 to take this over");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = want;
    register_ctx_stream(ctx, ctx->device, ctx->stream);
    return RTGL_OK;
}

extern "C" int rtgl_get_counters(rtgl_context *ctx, rtgl_counters *out)
{
    ENTER(ctx);
    if (!out) return fail(ctx, RTGL_ERR_INVALID, "out is NULL");
    if (!ctx->parts.empty()) {
        memset(out, 0, sizeof *out);
        for (rtgl_context *part : ctx->parts) {
            rtgl_counters c; const int rc = rtgl_get_counters(part, &c);
            if (rc) return fail(ctx, rc, part->error);
            out->paths += c.paths; out->segments += c.segments; out->triangle_tests += c.triangle_tests; out->candidates += c.candidates; out->env_lookups += c.env_lookups; out->culled_tests += c.culled_tests;
        }
        return RTGL_OK;
    }
    Counters c;
    HIPCHK(ctx, hipMemcpyAsync(&c, ctx->d_counters, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memset(out, 0, sizeof *out);
    out->paths = c.paths; out->segments = c.segments; out->triangle_tests = c.tri_tests;
    out->candidates = c.candidates; out->env_lookups = c.env_lookups; out->culled_tests = c.culled_tests;
    return RTGL_OK;
}

extern "C" int rtgl_read_rng_state(rtgl_context *ctx, uint32_t *xyzw)
{
    ENTER(ctx);
    if (!xyzw) return fail(ctx, RTGL_ERR_INVALID, "xyzw is NULL");
    if (!ctx->parts.empty()) {                          // rows from their owners, global row order
        std::vector<uint32_t> local;
        for (rtgl_context *part : ctx->parts) {
            local.resize(local_px(part) * 4);
            const int rc = rtgl_read_rng_state(part, local.data());
            if (rc) return fail(ctx, rc, part->error);
            for (int lr = 0; lr < part->local_rows; ++lr)
                memcpy(xyzw + (size_t)rtgl_local_row_to_global(part, lr) * ctx->width * 4, local.data() + (size_t)lr * ctx->width * 4, (size_t)ctx->width * 16);
        }
        return RTGL_OK;
    }
    if (!ctx->opt.rng_state || !ctx->d_rng) return fail(ctx, RTGL_ERR_STATE, "option rng_state was not enabled before rendering");
    return read_rows(ctx, xyzw, ctx->d_rng, 16);
}

// ---- first-hit planes (option "aov") ----------------------------------------------------------------
// plane bit -> index (0 albedo, 1 normal, 2 position, 3 ids); -1 for anything but one RTGL_AOV_* bit
static int aov_index(int plane)
{
    switch (plane) {
    case RTGL_AOV_ALBEDO: return 0;
    case RTGL_AOV_NORMAL: return 1;
    case RTGL_AOV_POSITION: return 2;
    case RTGL_AOV_IDS: return 3;
    default: return -1;
    }
}
static void *aov_plane(const rtgl_context *ctx, int idx) { return idx == 3 ? (void *)ctx->d_aov_ids : (void *)ctx->d_aov[idx]; }

// (re)allocate the enabled planes, zeroed; the mean restarts with the next frame.  The triangle ids are uploaded by the next frame.
static int set_aov(rtgl_context *ctx, int mask)
{
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // frames in flight may still write the old planes
    RCCHK(buf_release(ctx, ctx->d_aov[0], ctx->d_aov[1], ctx->d_aov[2], ctx->d_aov_ids));
    if (!(mask & RTGL_AOV_IDS)) {
        RCCHK(buf_release(ctx, ctx->d_visit_mesh, ctx->d_visit_tri));
        ctx->visit_ids_dirty = true;
    }
    ctx->opt.aov = 0;
    const size_t bytes = local_px(ctx) * 16;
    for (int k = 0; k < 4; ++k) {
        if (!(mask & (1 << k))) continue;
        RCCHK(k == 3 ? buf_alloc(ctx, ctx->d_aov_ids, bytes) : buf_alloc(ctx, ctx->d_aov[k], bytes));
        HIPCHK(ctx, hipMemsetAsync(aov_plane(ctx, k), 0, bytes, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->opt.aov = mask; ctx->aov_restart = true;
    return RTGL_OK;
}

extern "C" int rtgl_read_aov(rtgl_context *ctx, int plane, void *out)
{
    ENTER(ctx);
    const int idx = aov_index(plane);
    if (idx < 0) return fail(ctx, RTGL_ERR_INVALID, "plane must be one of RTGL_AOV_ALBEDO, RTGL_AOV_NORMAL, RTGL_AOV_POSITION, RTGL_AOV_IDS");
    if (!out) return fail(ctx, RTGL_ERR_INVALID, "out is NULL");
    const size_t row_bytes = (size_t)ctx->width * 16;
    if (!ctx->parts.empty()) {                          // rows from their owners, global row order
        std::vector<uint8_t> local;
        for (rtgl_context *part : ctx->parts) {
            local.resize(local_px(part) * 16);
            const int rc = rtgl_read_aov(part, plane, local.data());
            if (rc) return fail(ctx, rc, part->error);
            for (int lr = 0; lr < part->local_rows; ++lr)
                memcpy((uint8_t *)out + (size_t)rtgl_local_row_to_global(part, lr) * row_bytes, local.data() + (size_t)lr * row_bytes, row_bytes);
        }
        return RTGL_OK;
    }
    const void *src = aov_plane(ctx, idx);
    if (!src) return fail(ctx, RTGL_ERR_STATE, "this plane is not enabled (option \"aov\")");
    return read_rows(ctx, out, src, 16);
}

extern "C" void *rtgl_device_aov(rtgl_context *ctx, int plane)
{
    if (!ctx) return nullptr;
    if (!ctx->parts.empty()) { ctx->error = "rtgl_device_aov: a multi-device context holds its planes on every device; use rtgl_read_aov"; return nullptr; }
    const int idx = aov_index(plane);
    if (idx < 0) { ctx->error = "rtgl_device_aov: plane must be one RTGL_AOV_* bit"; return nullptr; }
    if (!aov_plane(ctx, idx)) { ctx->error = "rtgl_device_aov: this plane is not enabled (option \"aov\")"; return nullptr; }
    return aov_plane(ctx, idx);
}

// ---- guide pass (include/rtgl_amd.h, "guide pass"; kernel: rt_guides.hpp; host rules: rt_guides_plan.hpp) ---------------------------
static_assert(rt_guides_plan::kOk == (int)RTGL_OK && rt_guides_plan::kErrInvalid == (int)RTGL_ERR_INVALID && rt_guides_plan::kErrState == (int)RTGL_ERR_STATE
              && rt_guides_plan::kKernelSplit == (int)RTGL_KERNEL_WAVEFRONT_SPLIT && rt_guides_plan::kKernelSolo == (int)RTGL_KERNEL_WAVEFRONT_MFMA_SOLO, "the values of the header");

#include "rt_guides_host.hpp"

extern "C" int rtgl_guides_frame(rtgl_context *ctx)
{
    if (!ctx) return rt_guides_plan::refused(false, false, false, 0u).code;
    ENTER(ctx);
    const rt_guides_plan::Refusal refusal = rt_guides_plan::refused(true, !ctx->parts.empty(), ctx->have_params, (uint32_t)ctx->opt.aov);
    if (refusal.why) return fail(ctx, refusal.code, refusal.why);
    return guides_pass(ctx);
}

// ---- rtgl_denoise: edge-avoiding a-trous filter guided by the first-hit planes (rt_denoise.hpp) --------
static_assert(sizeof(rtgl_denoise_params) == sizeof(rt_denoise_plan::Params) && offsetof(rtgl_denoise_params, flags) == offsetof(rt_denoise_plan::Params, flags)
              && sizeof(rtgl_denoise_guided_params) == sizeof(rt_denoise_plan::GuidedParams) && offsetof(rtgl_denoise_guided_params, flags) == offsetof(rt_denoise_plan::GuidedParams, flags)
              && rt_denoise_plan::kFlagDemodulate == (uint32_t)RTGL_DENOISE_DEMODULATE && rt_denoise_plan::kPlaneAlbedo == (uint32_t)RTGL_AOV_ALBEDO
              && rt_denoise_plan::kPlaneNormal == (uint32_t)RTGL_AOV_NORMAL && rt_denoise_plan::kPlanePosition == (uint32_t)RTGL_AOV_POSITION
              && rt_denoise_plan::kPrepLdsBytes == kPrepLdsBytes, "the layouts of the header and of the kernels");

extern "C" int rtgl_denoise_defaults(rtgl_denoise_params *out)
{
    if (!out) return RTGL_ERR_INVALID;
    const rt_denoise_plan::Params p = rt_denoise_plan::default_params();
    memcpy(out, &p, sizeof p);
    return RTGL_OK;
}

// what the two denoisers filter: the accumulation image, or (option "denoise_source" = 1) the latest history buffer of
// rtgl_temporal_accumulate; NULL: there is none yet
static const float4 *denoise_input(const rtgl_context *ctx)
{
    if (ctx->opt.denoise_source == 0) return ctx->d_image;
    return ctx->has_temporal ? ctx->d_tm_hist[ctx->tm_cur] : nullptr;
}

// one pass: 64 columns x (four rows `step` apart) per block, two LDS buffers of nine arrays of 64 + 4 step floats (rt_denoise.hpp)
template <bool kDemod, bool kRemod>
static void launch_atrous(rtgl_context *ctx, const AtrousArgs &a)
{
    const rt_denoise_plan::Pass g = rt_denoise_plan::pass((uint32_t)a.step_log2, a.width, a.height);
    const dim3 grid(g.grid_x, g.grid_y);
    const size_t lds = rt_denoise_plan::lds_bytes(g, rt_denoise_plan::kAtrousArrays);
    if (g.wide) hipLaunchKernelGGL((atrous_kernel<kDemod, kRemod, true>), grid, dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL((atrous_kernel<kDemod, kRemod, false>), grid, dim3(256), lds, ctx->stream, a);
}

extern "C" int rtgl_denoise(rtgl_context *ctx, const rtgl_denoise_params *params)
{
    ENTER(ctx);
    rt_denoise_plan::Params P = rt_denoise_plan::default_params();
    if (params) memcpy(&P, params, sizeof P);
    if (const char *why = rt_denoise_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_denoise: ") + why);
    if (!ctx->parts.empty() || ctx->world > 1)
        return fail(ctx, RTGL_ERR_STATE, "rtgl_denoise: a tiled or multi-device context holds strips that lack their neighbours' rows; filtering a gathered image is out of scope: "
                                         "render on a single-device context, or filter the gathered image yourself");
    if (const char *why = rt_bucket_guide_plan::planes_refused(rt_denoise_plan::planes_needed(P), (uint32_t)ctx->opt.aov, ctx->aov_restart, ctx->aov_n))
        return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_denoise: ") + why);
    const size_t n = rt_denoise_plan::pixels(ctx->local_rows, ctx->width);
    if (const char *why = rt_denoise_plan::input_refused(n, ctx->opt.denoise_source, ctx->has_temporal)) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_denoise: ") + why);
    const float4 *input = denoise_input(ctx);
    const bool demod = (P.flags & RTGL_DENOISE_DEMODULATE) != 0, use_c = P.sigma_color > 0.0f, use_n = P.sigma_normal > 0.0f, use_p = P.sigma_position > 0.0f;
    // pass k of K reads the image (k = 0) or the buffer pass k - 1 wrote, and writes the denoised buffer (k = K - 1) or scratch k & 1
    RCCHK(buf_ensure(ctx, ctx->d_denoised, rt_denoise_plan::record_bytes(n)));
    for (uint32_t k = 0; k < rt_denoise_plan::scratch_buffers(P.passes); ++k) RCCHK(buf_ensure(ctx, ctx->d_dn_scratch[k], rt_denoise_plan::record_bytes(n)));
    AtrousArgs a{};
    a.albedo = demod ? ctx->d_aov[0] : nullptr; a.normal = use_n ? ctx->d_aov[1] : nullptr; a.position = use_p ? ctx->d_aov[2] : nullptr;
    a.width = ctx->width; a.height = ctx->local_rows;
    a.inv_normal = use_n ? 1.0f / (P.sigma_normal * P.sigma_normal) : 0.0f;
    a.sigma_position = P.sigma_position;
    a.use_color = use_c; a.use_normal = use_n; a.use_position = use_p;
    if (P.passes == 0u) {
        a.src = input; a.dst = ctx->d_denoised;
        const dim3 grid(rt_denoise_plan::identity_blocks(n));
        if (demod) hipLaunchKernelGGL(atrous_identity_kernel<true>, grid, dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(atrous_identity_kernel<false>, grid, dim3(256), 0, ctx->stream, a);
    }
    for (uint32_t k = 0; k < P.passes; ++k) {
        const bool first = k == 0u, last = k + 1u == P.passes;
        a.src = first ? input : ctx->d_dn_scratch[(k - 1u) & 1u];
        a.dst = last ? ctx->d_denoised : ctx->d_dn_scratch[k & 1u];
        a.step = 1 << k; a.step_log2 = (int)k;
        const float sig = P.sigma_color * ldexpf(1.0f, -(int)k);
        a.inv_color = use_c ? 1.0f / (sig * sig) : 0.0f;
        const bool dm = demod && first, rm = demod && last;
        if (dm && rm) launch_atrous<true, true>(ctx, a);
        else if (dm) launch_atrous<true, false>(ctx, a);
        else if (rm) launch_atrous<false, true>(ctx, a);
        else launch_atrous<false, false>(ctx, a);
    }
    HIPCHK(ctx, hipGetLastError());
    ctx->has_denoised = true;
    return RTGL_OK;
}

static const char *const kNoDenoise = ": no rtgl_denoise call has succeeded on this context";

extern "C" int rtgl_read_denoised_f32(rtgl_context *ctx, float *rgba)
{
    ENTER(ctx);
    return read_plane(ctx, rgba, "rgba is NULL", ctx->has_denoised, ctx->d_denoised, 16, "rtgl_read_denoised_f32", kNoDenoise);
}

extern "C" void *rtgl_device_denoised(rtgl_context *ctx)
{
    return ctx ? device_plane(ctx, ctx->has_denoised, ctx->d_denoised, "rtgl_device_denoised", kNoDenoise) : nullptr;
}

// ---- rtgl_denoise_guided: variance-guided a-trous filter with a firefly clamp (rt_denoise.hpp, guided_*) --------
extern "C" int rtgl_denoise_guided_defaults(rtgl_denoise_guided_params *out)
{
    if (!out) return RTGL_ERR_INVALID;
    const rt_denoise_plan::GuidedParams p = rt_denoise_plan::default_guided_params();
    memcpy(out, &p, sizeof p);
    return RTGL_OK;
}

// one guided pass: the geometry of launch_atrous with ten arrays per LDS buffer
template <bool kLast, bool kRemod>
static void launch_guided(rtgl_context *ctx, const GuidedArgs &a)
{
    const rt_denoise_plan::Pass g = rt_denoise_plan::pass((uint32_t)a.step_log2, a.width, a.height);
    const dim3 grid(g.grid_x, g.grid_y);
    const size_t lds = rt_denoise_plan::lds_bytes(g, rt_denoise_plan::kGuidedArrays);
    if (g.wide) hipLaunchKernelGGL((guided_kernel<kLast, kRemod, true>), grid, dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL((guided_kernel<kLast, kRemod, false>), grid, dim3(256), lds, ctx->stream, a);
}

// the guided passes behind a prepare kernel that wrote scratch 0: pass k of `passes` reads scratch k & 1 and writes scratch (k + 1) & 1 or,
// as the last, the denoised buffer; with every launch taken, the denoised and the variance buffers are there to read
static int launch_guided_passes(rtgl_context *ctx, GuidedArgs a, uint32_t passes, bool demod)
{
    for (uint32_t k = 0; k < passes; ++k) {
        const bool last = k + 1u == passes;
        a.src = ctx->d_dn_scratch[k & 1u];
        a.dst = last ? ctx->d_denoised : ctx->d_dn_scratch[(k + 1u) & 1u];
        a.step = 1 << k; a.step_log2 = (int)k;
        if (last && demod) launch_guided<true, true>(ctx, a);
        else if (last) launch_guided<true, false>(ctx, a);
        else launch_guided<false, false>(ctx, a);
    }
    HIPCHK(ctx, hipGetLastError());
    ctx->has_denoised = true; ctx->has_dn_variance = true;
    return RTGL_OK;
}

extern "C" int rtgl_denoise_guided(rtgl_context *ctx, const rtgl_denoise_guided_params *params)
{
    ENTER(ctx);
    rt_denoise_plan::GuidedParams P = rt_denoise_plan::default_guided_params();
    if (params) memcpy(&P, params, sizeof P);
    if (const char *why = rt_denoise_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_denoise_guided: ") + why);
    if (!ctx->parts.empty() || ctx->world > 1)
        return fail(ctx, RTGL_ERR_STATE, "rtgl_denoise_guided: a tiled or multi-device context holds strips that lack their neighbours' rows; filtering a gathered image is out of scope: "
                                         "render on a single-device context, or filter the gathered image yourself");
    if (const char *why = rt_bucket_guide_plan::planes_refused(rt_denoise_plan::planes_needed(P), (uint32_t)ctx->opt.aov, ctx->aov_restart, ctx->aov_n))
        return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_denoise_guided: ") + why);
    const size_t n = rt_denoise_plan::pixels(ctx->local_rows, ctx->width);
    if (const char *why = rt_denoise_plan::input_refused(n, ctx->opt.denoise_source, ctx->has_temporal)) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_denoise_guided: ") + why);
    const bool demod = (P.flags & RTGL_DENOISE_DEMODULATE) != 0, use_n = P.sigma_normal > 0.0f, use_p = P.sigma_position > 0.0f;
    if (const char *why = rt_denoise_plan::guided_variance_refused(ctx->opt.denoise_variance, ctx->opt.denoise_source, ctx->tm_moments, demod))
        return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_denoise_guided: ") + why);
    const float4 *input = denoise_input(ctx);
    const bool tvar = ctx->opt.denoise_variance == 1;
    // the prepare kernel writes scratch 0 (passes = 0: the denoised buffer); pass k of K reads scratch k & 1 and writes scratch (k + 1) & 1
    // or, as the last, the denoised buffer
    RCCHK(buf_ensure(ctx, ctx->d_denoised, rt_denoise_plan::record_bytes(n)));
    RCCHK(buf_ensure(ctx, ctx->d_dn_variance, rt_denoise_plan::record_bytes(n)));
    RCCHK(buf_ensure(ctx, ctx->d_dn_near, rt_denoise_plan::near_bytes(n)));
    for (uint32_t k = 0; k < rt_denoise_plan::guided_scratch_buffers(P.passes); ++k) RCCHK(buf_ensure(ctx, ctx->d_dn_scratch[k], rt_denoise_plan::record_bytes(n)));
    GuidedArgs a{};
    a.image = input; a.variance = ctx->d_dn_variance; a.near = ctx->d_dn_near;
    a.albedo = demod ? ctx->d_aov[0] : nullptr; a.normal = use_n ? ctx->d_aov[1] : nullptr; a.position = use_p ? ctx->d_aov[2] : nullptr;
    a.width = ctx->width; a.height = ctx->local_rows;
    a.lum2 = P.sigma_lum * P.sigma_lum;
    a.inv_normal = use_n ? 1.0f / (P.sigma_normal * P.sigma_normal) : 0.0f;
    a.sigma_position = P.sigma_position;
    a.firefly_ratio = P.firefly_ratio;
    a.use_clamp = P.firefly_ratio > 0.0f; a.use_normal = use_n; a.use_position = use_p;
    a.demodulate = demod; a.final_image = P.passes == 0u;
    a.dst = P.passes == 0u ? ctx->d_denoised : ctx->d_dn_scratch[0];
    const dim3 prep_grid(rt_denoise_plan::prepare_grid_x(a.width), rt_denoise_plan::prepare_grid_y(a.height));
    if (tvar) {
        GuidedTvarArgs t{};
        t.g = a; t.moments = ctx->d_tm_moments[ctx->tm_cur];
        hipLaunchKernelGGL(guided_prepare_tvar_kernel, prep_grid, dim3(256), kPrepLdsBytes, ctx->stream, t);
    } else hipLaunchKernelGGL(guided_prepare_kernel, prep_grid, dim3(256), kPrepLdsBytes, ctx->stream, a);
    return launch_guided_passes(ctx, a, P.passes, demod);
}

static const char *const kNoDenoiseGuided = ": no rtgl_denoise_guided call has succeeded on this context";

extern "C" int rtgl_read_denoise_variance_f32(rtgl_context *ctx, float *rgba)
{
    ENTER(ctx);
    return read_plane(ctx, rgba, "rgba is NULL", ctx->has_dn_variance, ctx->d_dn_variance, 16, "rtgl_read_denoise_variance_f32", kNoDenoiseGuided);
}

extern "C" void *rtgl_device_denoise_variance(rtgl_context *ctx)
{
    return ctx ? device_plane(ctx, ctx->has_dn_variance, ctx->d_dn_variance, "rtgl_device_denoise_variance", kNoDenoiseGuided) : nullptr;
}

// ---- rtgl_temporal_accumulate: reprojected history across camera moves (rt_temporal.hpp) --------
static_assert(sizeof(rtgl_temporal_params) == sizeof(rt_temporal_plan::Params) && offsetof(rtgl_temporal_params, flags) == offsetof(rt_temporal_plan::Params, flags)
              && sizeof(rtgl_temporal_clip_params) == sizeof(rt_temporal_plan::ClipParams) && offsetof(rtgl_temporal_clip_params, flags) == offsetof(rt_temporal_plan::ClipParams, flags)
              && rt_temporal_plan::kPlaneAlbedo == (uint32_t)RTGL_AOV_ALBEDO && rt_temporal_plan::kPlaneNormal == (uint32_t)RTGL_AOV_NORMAL
              && rt_temporal_plan::kPlanePosition == (uint32_t)RTGL_AOV_POSITION, "the layouts of the header");

extern "C" int rtgl_temporal_defaults(rtgl_temporal_params *out)
{
    if (!out) return RTGL_ERR_INVALID;
    const rt_temporal_plan::Params p = rt_temporal_plan::default_params();
    memcpy(out, &p, sizeof p);
    return RTGL_OK;
}

// the camera record of include/rtgl_amd.h ("temporal accumulation"): binary32, one rounding per operation, the tangent in double
static TemporalCamera temporal_camera(const FrameParams &P, int width, int height)
{
    auto dot = [](const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
    TemporalCamera c{};
    for (int k = 0; k < 3; ++k) { c.pos[k] = P.cam_pos[k]; c.fwd[k] = P.cam_forward[k]; c.up[k] = P.cam_up[k]; c.right[k] = P.cam_right[k]; }
    c.hw = (float)tan((double)P.cam_fov * 0.5);
    c.asp = (float)height / (float)width;
    c.wd = 2.0f * c.hw;
    c.ht = 2.0f * (c.hw * c.asp);
    c.ff = dot(c.fwd, c.fwd); c.rr = dot(c.right, c.right); c.uu = dot(c.up, c.up);
    c.kx = c.ff / (c.wd * c.rr);
    c.ky = c.ff / (c.ht * c.uu);
    return c;
}
static bool temporal_camera_equal(const TemporalCamera &a, const TemporalCamera &b)
{
    const float *x = a.pos, *y = b.pos;                   // (a NaN field compares unequal: no shortcut then)
    for (size_t k = 0; k < sizeof(TemporalCamera) / sizeof(float); ++k) if (!(x[k] == y[k])) return false;
    return true;
}

// kMom: option "temporal_moments"; its argument record is TemporalArgs (0) or TemporalMomentsArgs (1, 2)
template <int kMom, bool kHistory, bool kStatic>
static void launch_temporal(rtgl_context *ctx, const typename TemporalArgsOf<kMom>::type &a, bool use_n, bool use_p)
{
    const TemporalArgs &t = temporal_base(a);
    const dim3 grid(rt_temporal_plan::grid_x(t.width), rt_temporal_plan::grid_y(t.height));
    if (!kHistory) hipLaunchKernelGGL((temporal_kernel<false, false, false, false, kMom>), grid, dim3(256), 0, ctx->stream, a);
    else if (use_n && use_p) hipLaunchKernelGGL((temporal_kernel<true, kStatic, true, true, kMom>), grid, dim3(256), 0, ctx->stream, a);
    else if (use_n) hipLaunchKernelGGL((temporal_kernel<true, kStatic, true, false, kMom>), grid, dim3(256), 0, ctx->stream, a);
    else if (use_p) hipLaunchKernelGGL((temporal_kernel<true, kStatic, false, true, kMom>), grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL((temporal_kernel<true, kStatic, false, false, kMom>), grid, dim3(256), 0, ctx->stream, a);
}
template <int kMom>
static void launch_temporal(rtgl_context *ctx, const typename TemporalArgsOf<kMom>::type &a, bool history, bool at_rest, bool use_n, bool use_p)
{
    if (!history) launch_temporal<kMom, false, false>(ctx, a, use_n, use_p);
    else if (at_rest) launch_temporal<kMom, true, true>(ctx, a, use_n, use_p);
    else launch_temporal<kMom, true, false>(ctx, a, use_n, use_p);
}

extern "C" int rtgl_temporal_accumulate(rtgl_context *ctx, const rtgl_temporal_params *params)
{
    ENTER(ctx);
    rt_temporal_plan::Params P = rt_temporal_plan::default_params();
    if (params) memcpy(&P, params, sizeof P);
    if (const char *why = rt_temporal_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_temporal_accumulate: ") + why);
    if (!ctx->parts.empty() || ctx->world > 1)
        return fail(ctx, RTGL_ERR_STATE, "rtgl_temporal_accumulate: a tiled or multi-device context holds strips; a reprojected pixel may come from another strip, which is out of scope: "
                                         "render on a single-device context");
    const bool use_n = P.sigma_normal > 0.0f, use_p = P.sigma_position > 0.0f;
    const int moments = ctx->opt.temporal_moments;
    if (const char *why = rt_temporal_plan::planes_refused(rt_temporal_plan::planes_needed(P, moments), (uint32_t)ctx->opt.aov, ctx->aov_restart, ctx->aov_n, false))
        return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_temporal_accumulate: ") + why);
    const size_t n = rt_temporal_plan::pixels(ctx->local_rows, ctx->width);
    if (const char *why = rt_temporal_plan::pixels_refused(n)) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_temporal_accumulate: ") + why);
    const bool with_normal = (ctx->opt.aov & RTGL_AOV_NORMAL) != 0;      // the normal plane is copied whenever it is on, tested or not
    for (int k = 0; k < 2; ++k) {
        RCCHK(buf_ensure(ctx, ctx->d_tm_hist[k], rt_temporal_plan::record_bytes(n)));
        RCCHK(buf_ensure(ctx, ctx->d_tm_position[k], rt_temporal_plan::record_bytes(n)));
        if (with_normal) RCCHK(buf_ensure(ctx, ctx->d_tm_normal[k], rt_temporal_plan::record_bytes(n)));
        if (moments) RCCHK(buf_ensure(ctx, ctx->d_tm_moments[k], rt_temporal_plan::record_bytes(n)));
    }
    const TemporalCamera cam = temporal_camera(ctx->params, ctx->width, ctx->height);
    const bool history = rt_temporal_plan::history_usable(ctx->tm_valid, use_n, ctx->tm_has_normal);
    const int from = ctx->tm_cur, to = rt_temporal_plan::turn(ctx->has_temporal, from);             // the two sets take turns
    TemporalArgs a{};
    a.image = ctx->d_image; a.position = ctx->d_aov[2]; a.normal = with_normal ? ctx->d_aov[1] : nullptr;
    a.hist_prev = ctx->d_tm_hist[from]; a.position_prev = ctx->d_tm_position[from]; a.normal_prev = ctx->d_tm_normal[from];
    a.hist_out = ctx->d_tm_hist[to]; a.position_out = ctx->d_tm_position[to]; a.normal_out = ctx->d_tm_normal[to];
    a.width = ctx->width; a.height = ctx->local_rows;
    a.cur = cam; a.prev = ctx->tm_camera;
    a.max_history = P.max_history;
    a.inv_normal = use_n ? 1.0f / (P.sigma_normal * P.sigma_normal) : 0.0f;
    a.sigma_position = P.sigma_position;
    const bool at_rest = history && temporal_camera_equal(cam, ctx->tm_camera);
    if (moments) {                                        // (a change of the option dropped the history: what set `from` holds is of this mode)
        TemporalMomentsArgs m{};
        m.t = a; m.albedo = moments == 2 ? ctx->d_aov[0] : nullptr;
        m.mom_prev = ctx->d_tm_moments[from]; m.mom_out = ctx->d_tm_moments[to];
        if (moments == 2) launch_temporal<2>(ctx, m, history, at_rest, use_n, use_p);
        else launch_temporal<1>(ctx, m, history, at_rest, use_n, use_p);
    }
    else launch_temporal<0>(ctx, a, history, at_rest, use_n, use_p);
    HIPCHK(ctx, hipGetLastError());
    ctx->tm_moments = moments;
    ctx->tm_cur = to; ctx->tm_camera = cam; ctx->tm_has_normal = with_normal;
    ctx->tm_valid = true; ctx->has_temporal = true;
    return RTGL_OK;
}

extern "C" int rtgl_temporal_reset(rtgl_context *ctx)
{
    ENTER(ctx);
    ctx->tm_valid = false;                                // (the latest buffer stays readable)
    return RTGL_OK;
}

static const char *const kNoTemporal = ": no rtgl_temporal_accumulate call has succeeded on this context";
static const char *const kNoTemporalMoments = ": the latest successful rtgl_temporal_accumulate on this context stored no moments (option \"temporal_moments\")";

extern "C" int rtgl_read_temporal_f32(rtgl_context *ctx, float *rgba)
{
    ENTER(ctx);
    return read_plane(ctx, rgba, "rgba is NULL", ctx->has_temporal, ctx->d_tm_hist[ctx->tm_cur], 16, "rtgl_read_temporal_f32", kNoTemporal);
}

extern "C" void *rtgl_device_temporal(rtgl_context *ctx)
{
    return ctx ? device_plane(ctx, ctx->has_temporal, ctx->d_tm_hist[ctx->tm_cur], "rtgl_device_temporal", kNoTemporal) : nullptr;
}

extern "C" int rtgl_read_temporal_moments_f32(rtgl_context *ctx, float *rgba)
{
    ENTER(ctx);
    return read_plane(ctx, rgba, "rgba is NULL", ctx->tm_moments != 0, ctx->d_tm_moments[ctx->tm_cur], 16, "rtgl_read_temporal_moments_f32", kNoTemporalMoments);
}

extern "C" void *rtgl_device_temporal_moments(rtgl_context *ctx)
{
    return ctx ? device_plane(ctx, ctx->tm_moments != 0, ctx->d_tm_moments[ctx->tm_cur], "rtgl_device_temporal_moments", kNoTemporalMoments) : nullptr;
}

// ---- rtgl_temporal_clip: the latest history clamped into the current frame's neighbourhood colour box (rt_temporal_clip.hpp) --------
extern "C" int rtgl_temporal_clip_defaults(rtgl_temporal_clip_params *out)
{
    if (!out) return RTGL_ERR_INVALID;
    const rt_temporal_plan::ClipParams p = rt_temporal_plan::default_clip_params();
    memcpy(out, &p, sizeof p);
    return RTGL_OK;
}

template <bool kNormal, bool kPosition>
static void launch_temporal_clip(rtgl_context *ctx, const TemporalClipArgs &a, bool moments)
{
    const dim3 grid(rt_temporal_plan::grid_x(a.width), rt_temporal_plan::grid_y(a.height));
    if (moments) hipLaunchKernelGGL((temporal_clip_kernel<kNormal, kPosition, true>), grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL((temporal_clip_kernel<kNormal, kPosition, false>), grid, dim3(256), 0, ctx->stream, a);
}

extern "C" int rtgl_temporal_clip(rtgl_context *ctx, const rtgl_temporal_clip_params *params)
{
    ENTER(ctx);
    rt_temporal_plan::ClipParams P = rt_temporal_plan::default_clip_params();
    if (params) memcpy(&P, params, sizeof P);
    if (const char *why = rt_temporal_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_temporal_clip: ") + why);
    if (!ctx->parts.empty() || ctx->world > 1)
        return fail(ctx, RTGL_ERR_STATE, "rtgl_temporal_clip: a tiled or multi-device context holds strips that lack their neighbours' rows, and has no history (rtgl_temporal_accumulate is out of scope there): "
                                         "render on a single-device context");
    if (const char *why = rt_temporal_plan::clip_refused(ctx->has_temporal)) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_temporal_clip: ") + why);
    if (const char *why = rt_temporal_plan::planes_refused(rt_temporal_plan::planes_needed(P), (uint32_t)ctx->opt.aov, ctx->aov_restart, ctx->aov_n, true))
        return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_temporal_clip: ") + why);
    if (const char *why = rt_temporal_plan::pixels_refused(rt_temporal_plan::pixels(ctx->local_rows, ctx->width))) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_temporal_clip: ") + why);
    const bool use_n = P.sigma_normal > 0.0f, use_p = P.sigma_position > 0.0f;
    TemporalClipArgs a{};
    a.image = ctx->d_image; a.normal = use_n ? ctx->d_aov[1] : nullptr; a.position = ctx->d_aov[2];
    a.hist = ctx->d_tm_hist[ctx->tm_cur];
    a.moments = ctx->tm_moments ? ctx->d_tm_moments[ctx->tm_cur] : nullptr;
    a.width = ctx->width; a.height = ctx->local_rows;
    a.sigma_scale = P.sigma_scale; a.clip_history = P.clip_history;
    a.inv_normal = use_n ? 1.0f / (P.sigma_normal * P.sigma_normal) : 0.0f;
    a.sigma_position = P.sigma_position;
    const bool moments = ctx->tm_moments != 0;
    if (use_n && use_p) launch_temporal_clip<true, true>(ctx, a, moments);
    else if (use_n) launch_temporal_clip<true, false>(ctx, a, moments);
    else if (use_p) launch_temporal_clip<false, true>(ctx, a, moments);
    else launch_temporal_clip<false, false>(ctx, a, moments);
    HIPCHK(ctx, hipGetLastError());
    return RTGL_OK;
}

// ---- rtgl_tonemap: the display transform, float buffer -> RGBA8 (rt_tonemap.hpp) ----------------------------------------------------
static_assert(sizeof(rtgl_tonemap_params) == sizeof(rt_tonemap_plan::Params) && offsetof(rtgl_tonemap_params, adapt) == offsetof(rt_tonemap_plan::Params, adapt)
              && offsetof(rtgl_tonemap_params, low_permille) == offsetof(rt_tonemap_plan::Params, low_permille)
              && rt_tonemap_plan::kSourceImage == (uint32_t)RTGL_TONEMAP_SOURCE_IMAGE && rt_tonemap_plan::kSourceDenoised == (uint32_t)RTGL_TONEMAP_SOURCE_DENOISED
              && rt_tonemap_plan::kSourceTemporal == (uint32_t)RTGL_TONEMAP_SOURCE_TEMPORAL && rt_tonemap_plan::kOpLinear == (uint32_t)RTGL_TONEMAP_LINEAR
              && rt_tonemap_plan::kOpReinhard == (uint32_t)RTGL_TONEMAP_REINHARD && rt_tonemap_plan::kOpAces == (uint32_t)RTGL_TONEMAP_ACES
              && rt_tonemap_plan::kFlagAuto == (uint32_t)RTGL_TONEMAP_AUTO_EXPOSURE && rt_tonemap_plan::kBins == kToneBins && rt_tonemap_plan::kSetWords == kToneWords
              && rt_tonemap_plan::kExposureWord == kToneExposureWord && rt_tonemap_plan::kStateWords == kToneStateWords, "the layouts of the header and of the kernels");

extern "C" int rtgl_tonemap_defaults(rtgl_tonemap_params *out)
{
    if (!out) return RTGL_ERR_INVALID;
    const rt_tonemap_plan::Params p = rt_tonemap_plan::default_params();
    memcpy(out, &p, sizeof p);
    return RTGL_OK;
}

extern "C" int rtgl_tonemap(rtgl_context *ctx, const rtgl_tonemap_params *params)
{
    ENTER(ctx);
    rt_tonemap_plan::Params P = rt_tonemap_plan::default_params();
    if (params) memcpy(&P, params, sizeof P);
    if (const char *why = rt_tonemap_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_tonemap: ") + why);
    if (!ctx->parts.empty() || ctx->world > 1)
        return fail(ctx, RTGL_ERR_STATE, "rtgl_tonemap: a tiled or multi-device context holds strips, and the exposure is a property of the whole picture: render on a single-device context");
    if (const char *why = rt_tonemap_plan::source_refused(P.source, ctx->has_denoised, ctx->has_temporal)) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_tonemap: ") + why);
    const float4 *src = P.source == RTGL_TONEMAP_SOURCE_DENOISED ? ctx->d_denoised : P.source == RTGL_TONEMAP_SOURCE_TEMPORAL ? ctx->d_tm_hist[ctx->tm_cur] : ctx->d_image;
    const size_t n = (size_t)ctx->local_rows * ctx->width;
    if (const char *why = rt_tonemap_plan::pixels_refused(n)) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_tonemap: ") + why);
    RCCHK(buf_ensure(ctx, ctx->d_display, rt_tonemap_plan::display_bytes(n)));
    if (!ctx->d_tone_state) {
        RCCHK(buf_alloc(ctx, ctx->d_tone_state, kToneStateWords * 4));
        HIPCHK(ctx, hipMemsetAsync(ctx->d_tone_state, 0, kToneStateWords * 4, ctx->stream));      // both sets start clean; from here on the solve keeps them so
    }
    const bool automatic = rt_tonemap_plan::automatic(P);
    const unsigned blocks = rt_tonemap_plan::blocks(n, ctx->n_cus);
    if (automatic) {
        const int set = ctx->tone.set;
        hipLaunchKernelGGL(tonemap_histogram_kernel, dim3(blocks), dim3(256), 0, ctx->stream, src, n, ctx->d_tone_state + set * kToneWords);
        HIPCHK(ctx, hipGetLastError());
        TonemapSolveArgs s{};
        s.state = ctx->d_tone_state; s.set = set; s.use_prev = ctx->tone.prev ? 1u : 0u;
        s.low_permille = P.low_permille; s.high_permille = P.high_permille;
        s.exposure = P.exposure; s.key = P.key; s.adapt = P.adapt; s.exposure_min = P.exposure_min; s.exposure_max = P.exposure_max;
        hipLaunchKernelGGL(tonemap_solve_kernel, dim3(1), dim3(64), 0, ctx->stream, s);
        HIPCHK(ctx, hipGetLastError());
        ctx->tone.after_auto_call();
    }
    TonemapMapArgs a{};
    a.src = src; a.display = reinterpret_cast<uint32_t *>(ctx->d_display); a.n = n;
    a.exposure_word = automatic ? ctx->d_tone_state + kToneExposureWord : nullptr;
    a.exposure = P.exposure; a.white2 = P.white * P.white;
    if (P.op == RTGL_TONEMAP_LINEAR) hipLaunchKernelGGL(tonemap_map_kernel<0>, dim3(blocks), dim3(256), 0, ctx->stream, a);
    else if (P.op == RTGL_TONEMAP_REINHARD) hipLaunchKernelGGL(tonemap_map_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(tonemap_map_kernel<2>, dim3(blocks), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    ctx->has_display = true; ctx->tone_auto = automatic; ctx->tone_exposure = P.exposure;
    return RTGL_OK;
}

extern "C" int rtgl_tonemap_reset(rtgl_context *ctx)
{
    ENTER(ctx);
    ctx->tone.prev = false;                             // (the display buffer, the histogram and the exposure stay readable)
    return RTGL_OK;
}

extern "C" int rtgl_read_display_u8(rtgl_context *ctx, uint8_t *rgba, int flip)
{
    ENTER(ctx);
    if (!rgba) return fail(ctx, RTGL_ERR_INVALID, "rgba is NULL");
    if (!ctx->has_display) return fail(ctx, RTGL_ERR_STATE, "rtgl_read_display_u8: no rtgl_tonemap call has succeeded on this context");
    const size_t row = (size_t)ctx->width * 4, rows = (size_t)ctx->local_rows;
    if (!flip) return read_rows(ctx, rgba, ctx->d_display, 4);
    std::vector<uint8_t> tmp(rows * row);                 // the rows are turned over on the host: the device buffer keeps the image's order
    RCCHK(read_rows(ctx, tmp.data(), ctx->d_display, 4));
    for (size_t y = 0; y < rows; ++y) memcpy(rgba + (rows - 1 - y) * row, tmp.data() + y * row, row);
    return RTGL_OK;
}

extern "C" void *rtgl_device_display(rtgl_context *ctx)
{
    return ctx ? device_plane(ctx, ctx->has_display, ctx->d_display, "rtgl_device_display", ": no rtgl_tonemap call has succeeded on this context") : nullptr;
}

extern "C" int rtgl_read_tonemap_exposure(rtgl_context *ctx, float *exposure)
{
    ENTER(ctx);
    if (!exposure) return fail(ctx, RTGL_ERR_INVALID, "exposure is NULL");
    if (!ctx->has_display) return fail(ctx, RTGL_ERR_STATE, "rtgl_read_tonemap_exposure: no rtgl_tonemap call has succeeded on this context");
    if (!ctx->tone_auto) { *exposure = ctx->tone_exposure; return RTGL_OK; }
    HIPCHK(ctx, hipMemcpyAsync(exposure, ctx->d_tone_state + kToneExposureWord, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RTGL_OK;
}

extern "C" int rtgl_read_tonemap_histogram(rtgl_context *ctx, uint32_t hist[256], uint32_t *ignored)
{
    ENTER(ctx);
    if (!hist) return fail(ctx, RTGL_ERR_INVALID, "hist is NULL");
    if (ctx->tone.hist_set < 0) return fail(ctx, RTGL_ERR_STATE, "rtgl_read_tonemap_histogram: no rtgl_tonemap call with auto exposure has succeeded on this context");
    uint32_t words[kToneWords];
    HIPCHK(ctx, hipMemcpyAsync(words, ctx->d_tone_state + ctx->tone.hist_set * kToneWords, sizeof words, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(hist, words, kToneBins * 4);
    if (ignored) *ignored = words[kToneBins];
    return RTGL_OK;
}

// ---- rtgl_error_estimate: the noise level of the accumulation image and the stop rule (rt_error.hpp) -----------------------------------
static_assert(sizeof(rtgl_error_params) == sizeof(rt_error_plan::Params) && offsetof(rtgl_error_params, first_frames) == offsetof(rt_error_plan::Params, first_frames)
              && offsetof(rtgl_error_params, flags) == offsetof(rt_error_plan::Params, flags) && rt_error_plan::kFlagKeep == (uint32_t)RTGL_ERROR_KEEP_SNAPSHOT
              && rt_error_plan::kInvalid == RTGL_ERR_INVALID && rt_error_plan::kState == RTGL_ERR_STATE && rt_error_plan::kTile == (uint32_t)kErrTile
              && rt_error_plan::kSummaryBytes == kErrSummaryWords * 4 && rt_error_plan::kRecordBytes == sizeof(uint4), "the layouts of the header and of the kernels");

extern "C" int rtgl_error_defaults(rtgl_error_params *out)
{
    if (!out) return RTGL_ERR_INVALID;
    const rt_error_plan::Params p = rt_error_plan::default_params();
    memcpy(out, &p, sizeof p);
    return RTGL_OK;
}

extern "C" int rtgl_error_estimate(rtgl_context *ctx, const rtgl_error_params *params)
{
    ENTER(ctx);
    rt_error_plan::Params P = rt_error_plan::default_params();
    if (params) memcpy(&P, params, sizeof P);
    if (const char *why = rt_error_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_error_estimate: ") + why);
    if (!ctx->parts.empty() || ctx->world > 1)
        return fail(ctx, RTGL_ERR_STATE, "rtgl_error_estimate: a tiled or multi-device context holds strips, and the estimate is of the whole picture (out of scope): render on a single-device context");
    const rt_error_plan::Refusal no = rt_error_plan::refused(ctx->err, P, ctx->width, ctx->height);
    if (no.why) return fail(ctx, no.code, std::string("rtgl_error_estimate: ") + no.why);
    const unsigned tx = rt_error_plan::tiles_along(ctx->width), ty = rt_error_plan::tiles_along(ctx->height);
    RCCHK(buf_ensure(ctx, ctx->d_err_tiles, rt_error_plan::record_bytes(ctx->width, ctx->height)));
    RCCHK(buf_ensure(ctx, ctx->d_err_summary, rt_error_plan::kSummaryBytes));
    RCCHK(buf_ensure(ctx, ctx->d_err_snapshot, rt_error_plan::snapshot_bytes(ctx->width, ctx->height)));
    const rt_error_plan::Plan q = rt_error_plan::plan(ctx->err, P);
    ErrorTilesArgs a{};
    a.image = ctx->d_image; a.snapshot = ctx->d_err_snapshot; a.tiles = ctx->d_err_tiles;
    a.width = ctx->width; a.fw = (int)rt_error_plan::footprint_side(ctx->width); a.fh = (int)rt_error_plan::footprint_side(ctx->height);
    a.floor_ = P.floor; a.threshold = P.threshold;
    a.g_n = q.g_n; a.g_m = q.g_m; a.c = q.c;
    ErrorSolveArgs s{};
    s.tiles = ctx->d_err_tiles; s.summary = ctx->d_err_summary; s.n_tiles = tx * ty; s.valid = q.usable ? 1u : 0u;
    s.footprint = (uint32_t)rt_error_plan::footprint(ctx->width, ctx->height); s.quantile_permille = P.quantile_permille;
    s.c = q.c; s.frames_now = q.frames_now; s.frames_snapshot = q.frames_snapshot;
    const dim3 grid(tx, ty);
    if (!q.usable) hipLaunchKernelGGL((error_tiles_kernel<false, false>), grid, dim3(256), 0, ctx->stream, a);
    else if (q.keep) hipLaunchKernelGGL((error_tiles_kernel<true, true>), grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL((error_tiles_kernel<true, false>), grid, dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(error_solve_kernel, dim3(1), dim3(256), 0, ctx->stream, s);
    HIPCHK(ctx, hipGetLastError());
    rt_error_plan::taken(ctx->err, P, q.keep);
    ctx->has_error = true;
    return RTGL_OK;
}

extern "C" int rtgl_error_reset(rtgl_context *ctx)
{
    ENTER(ctx);
    rt_error_plan::drop(ctx->err);                        // (the summary and the tile records of the latest call stay readable)
    return RTGL_OK;
}

extern "C" int rtgl_read_error_summary(rtgl_context *ctx, rtgl_error_summary *out)
{
    ENTER(ctx);
    if (!out) return fail(ctx, RTGL_ERR_INVALID, "out is NULL");
    if (!ctx->has_error) return fail(ctx, RTGL_ERR_STATE, "rtgl_read_error_summary: no rtgl_error_estimate call has succeeded on this context");
    static_assert(sizeof(rtgl_error_summary) == kErrSummaryWords * 4 && sizeof(rtgl_error_params) == 32 && sizeof(rtgl_error_tile) == sizeof(uint4), "the layouts of the header");
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_err_summary, sizeof *out, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RTGL_OK;
}

extern "C" int rtgl_read_error_tiles(rtgl_context *ctx, rtgl_error_tile *tiles, uint32_t *tx, uint32_t *ty)
{
    ENTER(ctx);
    if (!tiles) return fail(ctx, RTGL_ERR_INVALID, "tiles is NULL");
    if (!ctx->has_error) return fail(ctx, RTGL_ERR_STATE, "rtgl_read_error_tiles: no rtgl_error_estimate call has succeeded on this context");
    const uint32_t nx = rt_error_plan::tiles_along(ctx->width), ny = rt_error_plan::tiles_along(ctx->height);
    HIPCHK(ctx, hipMemcpyAsync(tiles, ctx->d_err_tiles, (size_t)nx * ny * sizeof(rtgl_error_tile), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (tx) *tx = nx;
    if (ty) *ty = ny;
    return RTGL_OK;
}

extern "C" void *rtgl_device_error_tiles(rtgl_context *ctx)
{
    return ctx ? device_plane(ctx, ctx->has_error, ctx->d_err_tiles, "rtgl_device_error_tiles", ": no rtgl_error_estimate call has succeeded on this context") : nullptr;
}

// ---- adaptive sampling: masked frames over the tiles that are still noisy (rt_adaptive.hpp, rt_adaptive_plan.hpp) -------------------------
extern "C" int rtgl_adaptive_defaults(rtgl_adaptive_params *out)
{
    if (!out) return RTGL_ERR_INVALID;
    memset(out, 0, sizeof *out);
    out->threshold = 0.05f; out->floor = 0.01f; out->min_samples = 16u; out->max_samples = 1024u;
    return RTGL_OK;
}

static_assert(sizeof(rtgl_adaptive_params) == 32 && sizeof(rtgl_adaptive_tile) == sizeof(rt_adaptive_plan::Tile) && sizeof(rtgl_adaptive_summary) == sizeof(rt_adaptive_plan::Summary)
              && offsetof(rtgl_adaptive_summary, samples_total) == offsetof(rt_adaptive_plan::Summary, samples_total) && rt_adaptive_plan::kTile == kErrTile, "the layouts of the header");

// ---- a session of masked tiles on the host (TileSession): what rtgl_adaptive_* and rtgl_robust_adaptive_* both do, told neither kind.  `who`
// is the entry point's name and `no_session` its kind's wording, for the messages ------------------------------------------------------
static const char *const kNoAdaptiveSession = ": no session (rtgl_adaptive_begin has not been called, or the session has ended)";
static const char *const kNoRobustAdaptiveSession = ": no session (rtgl_robust_adaptive_begin has not been called, or rtgl_robust_adaptive_end has)";

// the mask as it stands -> its two lists on the device (the active blocks, then the active tiles); synchronises: the host vectors are free again
static int upload_tile_lists(rtgl_context *ctx, TileSession &s)
{
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    rt_adaptive_plan::build_lists(sh, s.mask, s.blocks, s.tiles);
    const size_t n_blocks = (size_t)sh.blocks_x * sh.blocks_y;
    if (!s.blocks.empty()) HIPCHK(ctx, hipMemcpyAsync(s.d_lists, s.blocks.data(), s.blocks.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (!s.tiles.empty()) HIPCHK(ctx, hipMemcpyAsync(s.d_lists + n_blocks, s.tiles.data(), s.tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RTGL_OK;
}

// a context that cannot hold a session is refused; otherwise the four buffers at its size (rt_robust_tiles_plan.hpp: a plane of samples, a
// record and two counts per tile, a word per block and per tile), where one that is live stays
static int tile_session_reserve(rtgl_context *ctx, TileSession &s, const char *who)
{
    if (!ctx->parts.empty() || ctx->world > 1)
        return fail(ctx, RTGL_ERR_STATE, std::string(who) + ": a tiled or multi-device context holds strips, and the tiles are the whole picture's (out of scope): render on a single-device context");
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    const size_t n_tiles = (size_t)sh.tx * sh.ty, n_blocks = (size_t)sh.blocks_x * sh.blocks_y;
    if ((uint64_t)n_blocks * 64ull > 0xFFFFFFF0ull) return fail(ctx, RTGL_ERR_INVALID, std::string(who) + ": the footprint does not fit 32-bit ray slots");
    RCCHK(buf_ensure(ctx, s.d_samples, rt_robust_tiles_plan::plane_bytes(rt_robust_tiles_plan::plane_pixels(ctx->width, ctx->height))));
    RCCHK(buf_ensure(ctx, s.d_records, rt_robust_tiles_plan::record_bytes(n_tiles)));
    RCCHK(buf_ensure(ctx, s.d_counts, rt_robust_tiles_plan::count_bytes(n_tiles)));
    RCCHK(buf_ensure(ctx, s.d_lists, rt_robust_tiles_plan::list_bytes(n_blocks, n_tiles)));
    return RTGL_OK;
}

// the reserved session opens: no record, no sample counted, every tile active and the lists on the device
static int tile_session_open(rtgl_context *ctx, TileSession &s)
{
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    const size_t n_tiles = (size_t)sh.tx * sh.ty;
    HIPCHK(ctx, hipMemsetAsync(s.d_records, 0, rt_robust_tiles_plan::record_bytes(n_tiles), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(s.d_counts, 0, rt_robust_tiles_plan::count_bytes(n_tiles), ctx->stream));
    rt_adaptive_plan::explicit_mask(sh, std::vector<uint8_t>(n_tiles, 1).data(), s.mask);
    RCCHK(upload_tile_lists(ctx, s));
    s.active = true;
    return RTGL_OK;
}

// the tail of an update, behind the kind's estimate kernel: the records it wrote to the host, the mask rule per tile, the lists of the new
// mask to the device, the summary
static int tile_session_update(rtgl_context *ctx, TileSession &s, uint32_t min_samples, uint32_t max_samples, rtgl_adaptive_summary *summary_out)
{
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    const size_t n_tiles = (size_t)sh.tx * sh.ty;
    std::vector<rt_adaptive_plan::Tile> records(n_tiles);
    HIPCHK(ctx, hipMemcpyAsync(records.data(), s.d_records, n_tiles * sizeof(rt_adaptive_plan::Tile), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t t = 0; t < (uint32_t)n_tiles; ++t) s.mask[t] = rt_adaptive_plan::active(sh, t, records[t], min_samples, max_samples) ? 1 : 0;
    RCCHK(upload_tile_lists(ctx, s));
    const rt_adaptive_plan::Summary sum = rt_adaptive_plan::summary(sh, records.data(), s.mask, (uint32_t)s.blocks.size(), max_samples);
    memcpy(summary_out, &sum, sizeof sum);
    return RTGL_OK;
}

static int tile_session_set_mask(rtgl_context *ctx, TileSession &s, const char *who, const char *no_session, const uint8_t *tiles)
{
    if (!tiles) return fail(ctx, RTGL_ERR_INVALID, std::string(who) + ": tiles is NULL");
    if (!s.active) return fail(ctx, RTGL_ERR_STATE, std::string(who) + no_session);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));       // (frames in flight read the lists about to be replaced)
    rt_adaptive_plan::explicit_mask(rt_adaptive_plan::shape(ctx->width, ctx->height), tiles, s.mask);
    return upload_tile_lists(ctx, s);
}

static int tile_session_get_mask(rtgl_context *ctx, const TileSession &s, const char *who, const char *no_session, uint8_t *tiles)
{
    if (!tiles) return fail(ctx, RTGL_ERR_INVALID, std::string(who) + ": tiles is NULL");
    if (!s.active) return fail(ctx, RTGL_ERR_STATE, std::string(who) + no_session);
    memcpy(tiles, s.mask.data(), s.mask.size());
    return RTGL_OK;
}

// the tile records and the tile grid; the caller has checked `tiles` and that the records are there
static int tile_session_read_tiles(rtgl_context *ctx, const TileSession &s, rtgl_adaptive_tile *tiles, uint32_t *tx, uint32_t *ty)
{
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    HIPCHK(ctx, hipMemcpyAsync(tiles, s.d_records, (size_t)sh.tx * sh.ty * sizeof(rtgl_adaptive_tile), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (tx) *tx = (uint32_t)sh.tx;
    if (ty) *ty = (uint32_t)sh.ty;
    return RTGL_OK;
}

// what a masked frame asks of the session and of the context; `no_params`: the kind's wording of the second refusal
static int masked_frame_refused(rtgl_context *ctx, const TileSession &s, const char *who, const char *no_session, const char *no_params)
{
    if (!s.active) return fail(ctx, RTGL_ERR_STATE, std::string(who) + no_session);
    if (!ctx->have_params) return fail(ctx, RTGL_ERR_STATE, no_params);
    if (ctx->opt.aov || ctx->opt.rng_state) return fail(ctx, RTGL_ERR_STATE, std::string(who) + ": a masked frame writes neither first-hit planes nor RNG states: options \"aov\" and \"rng_state\" must be 0");
    if (ctx->params.samples != 1u) return fail(ctx, RTGL_ERR_INVALID, std::string(who) + ": a masked frame is one sample per pixel: samples must be 1");
    if (ctx->params.max_bounce == 0u) return fail(ctx, RTGL_ERR_INVALID, std::string(who) + ": max_bounce must be > 0");
    return RTGL_OK;
}

extern "C" int rtgl_adaptive_begin(rtgl_context *ctx, const rtgl_adaptive_params *params)
{
    ENTER(ctx);
    if (!params) return fail(ctx, RTGL_ERR_INVALID, "rtgl_adaptive_begin: params is NULL");
    const rtgl_adaptive_params P = *params;
    for (float v : { P.threshold, P.floor })
        if (!std::isfinite(v) || !(v > 0.0f)) return fail(ctx, RTGL_ERR_INVALID, "rtgl_adaptive_begin: threshold and floor must be finite and > 0");
    if (P.min_samples < 1u || P.max_samples < P.min_samples) return fail(ctx, RTGL_ERR_INVALID, "rtgl_adaptive_begin: 1 <= min_samples <= max_samples is required");
    if (P.flags) return fail(ctx, RTGL_ERR_INVALID, "rtgl_adaptive_begin: no flag is defined");
    for (uint32_t r : P.reserved) if (r) return fail(ctx, RTGL_ERR_INVALID, "rtgl_adaptive_begin: reserved fields must be 0");
    RCCHK(tile_session_reserve(ctx, ctx->ad, "rtgl_adaptive_begin"));
    ctx->ad.active = false;
    RCCHK(buf_ensure(ctx, ctx->d_ad_snapshot, (size_t)ctx->height * ctx->width * sizeof(float)));
    // the image as rtgl_clear_image leaves it
    HIPCHK(ctx, hipMemsetAsync(ctx->d_image, 0, (size_t)ctx->local_rows * ctx->width * 16, ctx->stream));
    ctx->aov_restart = true;
    rt_error_plan::drop(ctx->err);
    ctx->ad_params = P; ctx->has_adaptive = true;
    return tile_session_open(ctx, ctx->ad);
}

// One masked frame (rt_adaptive.hpp): the blocks of `list` (n0 = 64 x its length > 0) traced as a one-frame image into `samples`, from the
// start event of rtgl_last_frame_ms up to the last kernel of the pipeline.  The caller has checked the frame parameters; it folds the
// sample buffer and records the end event.
static int masked_frame(rtgl_context *ctx, float4 *samples, const uint32_t *list, uint32_t n0)
{
    if (ctx->visits_dirty) RCCHK(rebuild_sphere_visits(ctx));
    if (ctx->tris_dirty) RCCHK(rebuild_triangles(ctx));
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    const SceneView sc = scene_view(ctx);
    // a one-frame image in the sample buffer: accumulate_pixel stores (radiance + 0 x 0) / 1
    std::vector<FrameParams> frames(1, ctx->params);
    FrameParams &P = frames[0];
    if (!ctx->d_env) P.use_envmap = 0;
    P.frames = 0; P.reset_flag = 1;
    ImageView im{};
    im.pixels = samples; im.width = ctx->width; im.height = ctx->height;
    im.disp_w = sh.fw; im.disp_h = sh.fh;
    im.local_rows = ctx->local_rows; im.rank = ctx->rank; im.world = ctx->world; im.strip_rows = ctx->strip_rows;
    if (ctx->opt.counters) HIPCHK(ctx, hipMemsetAsync(ctx->d_counters, 0, sizeof(Counters), ctx->stream));
    // the per-bounce pipeline whatever the scene: where an ordinary frame would take the megakernel, RTGL_KERNEL_WAVEFRONT
    const int effective = (ctx->n_tri_visits == 0 && !ctx->kernel_explicit) ? (int)RTGL_KERNEL_MEGA : ctx->opt.kernel;
    const int saved_kernel = ctx->opt.kernel;
    ctx->opt.kernel = effective == RTGL_KERNEL_MEGA ? (int)RTGL_KERNEL_WAVEFRONT : effective;
    ctx->kernel_in_use = ctx->opt.kernel;
    int rc = ensure_wave_buffers(ctx, n0, P.max_bounce, false);
    if (!rc) {
        ctx->wb.batch_rad = nullptr; ctx->wb.batch_px = 0;
        ctx->last_batch_frames = 1;
        ctx->timing_this_frame = false;                   // (option "kernel_timing" covers ordinary frames)
        rc = (int)hipEventRecord(ctx->ev0, ctx->stream) ? fail(ctx, RTGL_ERR_DEVICE, "hipEventRecord failed") : RTGL_OK;
    }
    if (!rc) {
        rc = launch_wavefront(ctx, sc, frames, im, n0, nullptr, nullptr, list);
        if (rc) ctx->keep0_valid = false;                 // (as in render_batch: a frame that failed half way vouches for nothing it left behind)
    }
    ctx->opt.kernel = saved_kernel;
    return rc;
}

extern "C" int rtgl_adaptive_frame(rtgl_context *ctx)
{
    ENTER(ctx);
    RCCHK(masked_frame_refused(ctx, ctx->ad, "rtgl_adaptive_frame", kNoAdaptiveSession, "rtgl_set_frame_params has not been called"));
    rt_error_plan::drop(ctx->err);                        // (rtgl_error_estimate: the image is no longer one accumulation of counted frames)
    if (ctx->ad.blocks.empty()) return RTGL_OK;
    RCCHK(masked_frame(ctx, ctx->ad.d_samples, ctx->ad.d_lists, (uint32_t)ctx->ad.blocks.size() * 64u));
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    AdaptiveMergeArgs a{};
    a.image = ctx->d_image; a.samples = ctx->ad.d_samples; a.n = ctx->ad.d_counts;
    a.tiles = ctx->ad.d_lists + (size_t)sh.blocks_x * sh.blocks_y;
    a.width = ctx->width; a.fw = sh.fw; a.fh = sh.fh; a.tx = sh.tx;
    hipLaunchKernelGGL(adaptive_merge_kernel, dim3((unsigned)ctx->ad.tiles.size()), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    return RTGL_OK;
}

extern "C" int rtgl_adaptive_update(rtgl_context *ctx, rtgl_adaptive_summary *summary_out)
{
    ENTER(ctx);
    if (!summary_out) return fail(ctx, RTGL_ERR_INVALID, "rtgl_adaptive_update: summary_out is NULL");
    if (!ctx->ad.active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_adaptive_update") + kNoAdaptiveSession);
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    AdaptiveTilesArgs a{};
    a.image = ctx->d_image; a.snapshot = ctx->d_ad_snapshot; a.records = ctx->ad.d_records;
    a.n = ctx->ad.d_counts; a.m = ctx->ad.d_counts + (size_t)sh.tx * sh.ty;
    a.width = ctx->width; a.fw = sh.fw; a.fh = sh.fh;
    a.floor_ = ctx->ad_params.floor; a.threshold = ctx->ad_params.threshold;
    hipLaunchKernelGGL(adaptive_tiles_kernel, dim3((unsigned)sh.tx, (unsigned)sh.ty), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return tile_session_update(ctx, ctx->ad, ctx->ad_params.min_samples, ctx->ad_params.max_samples, summary_out);
}

extern "C" int rtgl_adaptive_set_mask(rtgl_context *ctx, const uint8_t *tiles)
{
    ENTER(ctx);
    return tile_session_set_mask(ctx, ctx->ad, "rtgl_adaptive_set_mask", kNoAdaptiveSession, tiles);
}

extern "C" int rtgl_adaptive_get_mask(rtgl_context *ctx, uint8_t *tiles)
{
    ENTER(ctx);
    return tile_session_get_mask(ctx, ctx->ad, "rtgl_adaptive_get_mask", kNoAdaptiveSession, tiles);
}

extern "C" int rtgl_read_adaptive_tiles(rtgl_context *ctx, rtgl_adaptive_tile *tiles, uint32_t *tx, uint32_t *ty)
{
    ENTER(ctx);
    if (!tiles) return fail(ctx, RTGL_ERR_INVALID, "tiles is NULL");
    if (!ctx->has_adaptive) return fail(ctx, RTGL_ERR_STATE, "rtgl_read_adaptive_tiles: no rtgl_adaptive_begin call has succeeded on this context");
    return tile_session_read_tiles(ctx, ctx->ad, tiles, tx, ty);
}

extern "C" void *rtgl_device_adaptive_tiles(rtgl_context *ctx)
{
    return ctx ? device_plane(ctx, ctx->has_adaptive, ctx->ad.d_records, "rtgl_device_adaptive_tiles", ": no rtgl_adaptive_begin call has succeeded on this context") : nullptr;
}

// ---- robust accumulation: K bucket means and a Gini-trimmed resolve (rt_robust.hpp, rt_robust_plan.hpp) -----------------------------------
static_assert(sizeof(rtgl_robust_params) == sizeof(rt_robust_plan::Params) && sizeof(rtgl_robust_resolve_params) == sizeof(rt_robust_plan::ResolveParams)
              && offsetof(rtgl_robust_resolve_params, dest) == offsetof(rt_robust_plan::ResolveParams, dest) && (uint32_t)RTGL_ROBUST_DEST_BUFFER == rt_robust_plan::kDestBuffer
              && (uint32_t)RTGL_ROBUST_DEST_IMAGE == rt_robust_plan::kDestImage, "the layouts of the header");

extern "C" int rtgl_robust_defaults(rtgl_robust_params *params, rtgl_robust_resolve_params *resolve_params)
{
    if (!params && !resolve_params) return RTGL_ERR_INVALID;
    if (params) { const rt_robust_plan::Params p = rt_robust_plan::default_params(); memcpy(params, &p, sizeof p); }
    if (resolve_params) { const rt_robust_plan::ResolveParams p = rt_robust_plan::default_resolve_params(); memcpy(resolve_params, &p, sizeof p); }
    return RTGL_OK;
}

extern "C" int rtgl_robust_begin(rtgl_context *ctx, const rtgl_robust_params *params)
{
    ENTER(ctx);
    if (!params) return fail(ctx, RTGL_ERR_INVALID, "rtgl_robust_begin: params is NULL");
    rt_robust_plan::Params P;
    memcpy(&P, params, sizeof P);
    if (const char *why = rt_robust_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_robust_begin: ") + why);
    if (!ctx->parts.empty())
        return fail(ctx, RTGL_ERR_STATE, "rtgl_robust_begin: a multi-device context holds its rows on several devices (out of scope): accumulate on a single-device or a tiled context");
    const size_t px = rt_robust_plan::plane_pixels(ctx->local_rows, ctx->width);
    ctx->rb_active = false;
    if (ctx->rb_K != P.buckets) { RCCHK(buf_release(ctx, ctx->d_rb_buckets)); ctx->rb_K = 0; }
    RCCHK(buf_ensure(ctx, ctx->d_rb_buckets, rt_robust_plan::bucket_bytes(px, P.buckets)));
    ctx->rb_K = P.buckets;
    RCCHK(buf_ensure(ctx, ctx->d_rb_out, rt_robust_plan::output_bytes(px)));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_rb_buckets, 0, rt_robust_plan::bucket_bytes(px, P.buckets), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_rb_out, 0, rt_robust_plan::output_bytes(px), ctx->stream));
    ctx->rb_N = 0; ctx->rb_resolved = false; ctx->has_rb_error = false; ctx->rb_active = true;      // (the records of rtgl_robust_error_estimate stay allocated)
    return RTGL_OK;
}

static const char *const kNoRobustSession = ": no session (rtgl_robust_begin has not been called, or rtgl_robust_end has)";

extern "C" int rtgl_robust_accumulate(rtgl_context *ctx)
{
    ENTER(ctx);
    if (!ctx->rb_active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_accumulate") + kNoRobustSession);
    if (ctx->rb_N == rt_robust_plan::kMaxFrames) return fail(ctx, RTGL_ERR_STATE, "rtgl_robust_accumulate: the frame count is 32 bits wide");
    const size_t px = rt_robust_plan::plane_pixels(ctx->local_rows, ctx->width), n = (size_t)ctx->local_rows * ctx->width;
    if (n) {
        hipLaunchKernelGGL(robust_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const float4 *)ctx->d_image,
                           ctx->d_rb_buckets + (size_t)rt_robust_plan::next_bucket(ctx->rb_N, ctx->rb_K) * px, rt_robust_plan::next_count(ctx->rb_N, ctx->rb_K), (uint32_t)n);
        HIPCHK(ctx, hipGetLastError());
    }
    ctx->rb_N++;
    return RTGL_OK;
}

// f(K) with a session's bucket count as a compile-time constant, for the <4>, <8> and <16> instantiations of a kernel.  The count is one
// that *_plan::invalid let through at begin; with any other, nothing is launched
template <typename F>
static void with_buckets(uint32_t K, F &&f)
{
    if (K == 4u) f(std::integral_constant<int, 4>{});
    else if (K == 8u) f(std::integral_constant<int, 8>{});
    else if (K == 16u) f(std::integral_constant<int, 16>{});
}

extern "C" int rtgl_robust_resolve(rtgl_context *ctx, const rtgl_robust_resolve_params *params)
{
    ENTER(ctx);
    if (!params) return fail(ctx, RTGL_ERR_INVALID, "rtgl_robust_resolve: params is NULL");
    rt_robust_plan::ResolveParams P;
    memcpy(&P, params, sizeof P);
    if (const char *why = rt_robust_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_robust_resolve: ") + why);
    if (!ctx->rb_active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_resolve") + kNoRobustSession);
    if (ctx->rb_N == 0u) return fail(ctx, RTGL_ERR_STATE, "rtgl_robust_resolve: no frame has been accumulated since rtgl_robust_begin");
    const bool to_image = P.dest == rt_robust_plan::kDestImage;
    if (to_image) {                                       // on the host, what rtgl_write_image_f32 does
        rt_error_plan::drop(ctx->err);                    // (rtgl_error_estimate: another image, the snapshot is dropped)
        ctx->ad.active = false;                           // (adaptive sampling: ... and the session ends)
    }
    RobustResolveArgs a{};
    a.buckets = ctx->d_rb_buckets; a.out = to_image ? ctx->d_image : ctx->d_rb_out;
    a.plane = rt_robust_plan::plane_pixels(ctx->local_rows, ctx->width); a.n = (uint32_t)((size_t)ctx->local_rows * ctx->width);
    a.frames = ctx->rb_N; a.gain = P.gain;
    if (a.n) {
        const dim3 grid((unsigned)((a.n + 255u) / 256u));
        with_buckets(ctx->rb_K, [&](auto K) {
            if (to_image) hipLaunchKernelGGL((robust_resolve_kernel<K, 1>), grid, dim3(256), 0, ctx->stream, a);
            else hipLaunchKernelGGL((robust_resolve_kernel<K, 0>), grid, dim3(256), 0, ctx->stream, a);
        });
        HIPCHK(ctx, hipGetLastError());
    }
    if (!to_image) ctx->rb_resolved = true;
    return RTGL_OK;
}

extern "C" int rtgl_robust_end(rtgl_context *ctx)
{
    ENTER(ctx);
    if (!ctx->rb_active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_end") + kNoRobustSession);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // (folds and resolves in flight use the planes)
    ctx->rb_active = false; ctx->rb_resolved = false; ctx->has_rb_error = false; ctx->rb_K = 0; ctx->rb_N = 0;
    return buf_release(ctx, ctx->d_rb_buckets, ctx->d_rb_out, ctx->d_rbe_tiles, ctx->d_rbe_summary);
}

extern "C" int rtgl_robust_frames(rtgl_context *ctx, uint32_t *frames, uint32_t *buckets)
{
    ENTER_NOFLUSH(ctx);
    if (!frames && !buckets) return fail(ctx, RTGL_ERR_INVALID, "rtgl_robust_frames: both pointers are NULL");
    if (!ctx->rb_active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_frames") + kNoRobustSession);
    if (frames) *frames = ctx->rb_N;
    if (buckets) *buckets = ctx->rb_K;
    return RTGL_OK;
}

extern "C" int rtgl_read_robust_f32(rtgl_context *ctx, float *rgba)
{
    ENTER(ctx);
    if (!rgba) return fail(ctx, RTGL_ERR_INVALID, "rgba is NULL");
    if (!ctx->rb_active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_read_robust_f32") + kNoRobustSession);
    if (!ctx->rb_resolved) return fail(ctx, RTGL_ERR_STATE, "rtgl_read_robust_f32: no rtgl_robust_resolve with dest RTGL_ROBUST_DEST_BUFFER since rtgl_robust_begin");
    return read_rows(ctx, rgba, ctx->d_rb_out, 16);
}

extern "C" int rtgl_read_robust_bucket_f32(rtgl_context *ctx, uint32_t bucket, float *rgba)
{
    ENTER(ctx);
    if (!rgba) return fail(ctx, RTGL_ERR_INVALID, "rgba is NULL");
    if (!ctx->rb_active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_read_robust_bucket_f32") + kNoRobustSession);
    if (bucket >= ctx->rb_K) return fail(ctx, RTGL_ERR_INVALID, "rtgl_read_robust_bucket_f32: bucket >= buckets");
    return read_rows(ctx, rgba, ctx->d_rb_buckets + (size_t)bucket * rt_robust_plan::plane_pixels(ctx->local_rows, ctx->width), 16);
}

// ---- rtgl_robust_error_estimate: the noise level of the picture a session's resolve makes (rt_spread.hpp, rt_spread_plan.hpp) -------------
static_assert(sizeof(rtgl_robust_error_params) == sizeof(rt_spread_plan::Params) && offsetof(rtgl_robust_error_params, quantile_permille) == offsetof(rt_spread_plan::Params, quantile_permille)
              && rt_spread_plan::kSummaryBytes == kErrSummaryWords * 4 && rt_spread_plan::kRecordBytes == sizeof(uint4) && rt_spread_plan::kTile == (uint32_t)kErrTile, "the layouts of the header");

extern "C" int rtgl_robust_error_defaults(rtgl_robust_error_params *out)
{
    if (!out) return RTGL_ERR_INVALID;
    const rt_spread_plan::Params p = rt_spread_plan::default_params();
    memcpy(out, &p, sizeof p);
    return RTGL_OK;
}

extern "C" int rtgl_robust_error_estimate(rtgl_context *ctx, const rtgl_robust_error_params *params)
{
    ENTER(ctx);
    rt_spread_plan::Params P = rt_spread_plan::default_params();
    if (params) memcpy(&P, params, sizeof P);
    if (const char *why = rt_spread_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_robust_error_estimate: ") + why);
    if (!ctx->parts.empty() || ctx->world > 1)
        return fail(ctx, RTGL_ERR_STATE, "rtgl_robust_error_estimate: a tiled or multi-device context holds strips, and the estimate is of the whole picture (out of scope): render on a single-device context");
    if (const char *why = rt_spread_plan::refused(ctx->rb_active, ctx->rb_N, ctx->rb_K)) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_error_estimate: ") + why);
    if (!rt_spread_plan::footprint_fits(ctx->width, ctx->height)) return fail(ctx, RTGL_ERR_INVALID, "rtgl_robust_error_estimate: the footprint does not fit 32-bit counts");
    const unsigned tx = rt_spread_plan::tiles_along(ctx->width), ty = rt_spread_plan::tiles_along(ctx->height);
    RCCHK(buf_ensure(ctx, ctx->d_rbe_tiles, rt_spread_plan::record_bytes(ctx->width, ctx->height)));
    RCCHK(buf_ensure(ctx, ctx->d_rbe_summary, rt_spread_plan::kSummaryBytes));
    SpreadTilesArgs a{};
    a.buckets = ctx->d_rb_buckets; a.tiles = ctx->d_rbe_tiles; a.plane = rt_robust_plan::plane_pixels(ctx->local_rows, ctx->width);
    a.width = ctx->width; a.fw = (int32_t)rt_spread_plan::footprint_side(ctx->width); a.fh = (int32_t)rt_spread_plan::footprint_side(ctx->height);
    a.gain = P.gain; a.floor_ = P.floor; a.threshold = P.threshold;
    ErrorSolveArgs s{};
    s.tiles = ctx->d_rbe_tiles; s.summary = ctx->d_rbe_summary; s.n_tiles = tx * ty; s.valid = 1u;
    s.frames_now = (int32_t)ctx->rb_N; s.frames_snapshot = 0;
    s.footprint = (uint32_t)rt_spread_plan::footprint(ctx->width, ctx->height); s.quantile_permille = P.quantile_permille; s.c = 1.0f;
    const dim3 grid(tx, ty);
    with_buckets(ctx->rb_K, [&](auto K) { hipLaunchKernelGGL(spread_tiles_kernel<K>, grid, dim3(256), 0, ctx->stream, a); });
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(error_solve_kernel, dim3(1), dim3(256), 0, ctx->stream, s);
    HIPCHK(ctx, hipGetLastError());
    ctx->has_rb_error = true;
    return RTGL_OK;
}

static const char *const kNoRobustError = ": no rtgl_robust_error_estimate call has succeeded in this session";

extern "C" int rtgl_read_robust_error_summary(rtgl_context *ctx, rtgl_error_summary *out)
{
    ENTER(ctx);
    if (!out) return fail(ctx, RTGL_ERR_INVALID, "out is NULL");
    if (!ctx->rb_active || !ctx->has_rb_error) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_read_robust_error_summary") + kNoRobustError);
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_rbe_summary, sizeof *out, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RTGL_OK;
}

extern "C" int rtgl_read_robust_error_tiles(rtgl_context *ctx, rtgl_error_tile *tiles, uint32_t *tx, uint32_t *ty)
{
    ENTER(ctx);
    if (!tiles) return fail(ctx, RTGL_ERR_INVALID, "tiles is NULL");
    if (!ctx->rb_active || !ctx->has_rb_error) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_read_robust_error_tiles") + kNoRobustError);
    const uint32_t nx = rt_spread_plan::tiles_along(ctx->width), ny = rt_spread_plan::tiles_along(ctx->height);
    HIPCHK(ctx, hipMemcpyAsync(tiles, ctx->d_rbe_tiles, (size_t)nx * ny * sizeof(rtgl_error_tile), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (tx) *tx = nx;
    if (ty) *ty = ny;
    return RTGL_OK;
}

extern "C" void *rtgl_device_robust_error_tiles(rtgl_context *ctx)
{
    return ctx ? device_plane(ctx, ctx->rb_active && ctx->has_rb_error, ctx->d_rbe_tiles, "rtgl_device_robust_error_tiles", kNoRobustError) : nullptr;
}

// ---- a robust adaptive session: masked frames folded into per-tile bucket means (rt_robust_tiles.hpp, rt_robust_tiles_plan.hpp) ------------
static_assert(sizeof(rtgl_robust_adaptive_params) == sizeof(rt_robust_tiles_plan::Params) && offsetof(rtgl_robust_adaptive_params, gain) == offsetof(rt_robust_tiles_plan::Params, gain)
              && offsetof(rtgl_robust_adaptive_params, max_samples) == offsetof(rt_robust_tiles_plan::Params, max_samples), "the layouts of the header");

extern "C" int rtgl_robust_adaptive_defaults(rtgl_robust_adaptive_params *out)
{
    if (!out) return RTGL_ERR_INVALID;
    const rt_robust_tiles_plan::Params p = rt_robust_tiles_plan::default_params();
    memcpy(out, &p, sizeof p);
    return RTGL_OK;
}

extern "C" int rtgl_robust_adaptive_begin(rtgl_context *ctx, const rtgl_robust_adaptive_params *params)
{
    ENTER(ctx);
    if (!params) return fail(ctx, RTGL_ERR_INVALID, "rtgl_robust_adaptive_begin: params is NULL");
    rt_robust_tiles_plan::Params P;
    memcpy(&P, params, sizeof P);
    if (const char *why = rt_robust_tiles_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_robust_adaptive_begin: ") + why);
    RCCHK(tile_session_reserve(ctx, ctx->ra, "rtgl_robust_adaptive_begin"));
    const size_t px = rt_robust_tiles_plan::plane_pixels(ctx->width, ctx->height);
    if (ctx->ra.active) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // (work in flight uses the planes and the lists)
    ctx->ra.active = false; ctx->ra_resolved = false;
    if (ctx->ra_K != P.buckets) { RCCHK(buf_release(ctx, ctx->d_ra_buckets)); ctx->ra_K = 0; }
    RCCHK(buf_ensure(ctx, ctx->d_ra_buckets, rt_robust_tiles_plan::bucket_bytes(px, P.buckets)));
    ctx->ra_K = P.buckets;
    RCCHK(buf_ensure(ctx, ctx->d_ra_out, rt_robust_tiles_plan::plane_bytes(px)));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_ra_buckets, 0, rt_robust_tiles_plan::bucket_bytes(px, P.buckets), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->ra.d_samples, 0, rt_robust_tiles_plan::plane_bytes(px), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_ra_out, 0, rt_robust_tiles_plan::plane_bytes(px), ctx->stream));
    ctx->ra_params = P;
    return tile_session_open(ctx, ctx->ra);
}

// the fold of `source` into the bucket of every active tile's next sample; nothing with an empty list
static int robust_adaptive_fold(rtgl_context *ctx, const float4 *source)
{
    if (ctx->ra.tiles.empty()) return RTGL_OK;
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    TileBucketsFoldArgs a{};
    a.source = source; a.buckets = ctx->d_ra_buckets; a.plane = rt_robust_tiles_plan::plane_pixels(ctx->width, ctx->height);
    a.n = ctx->ra.d_counts; a.tiles = ctx->ra.d_lists + (size_t)sh.blocks_x * sh.blocks_y; a.K = ctx->ra_K;
    a.width = ctx->width; a.fw = sh.fw; a.fh = sh.fh; a.tx = sh.tx;
    hipLaunchKernelGGL(tile_buckets_fold_kernel, dim3((unsigned)ctx->ra.tiles.size()), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return RTGL_OK;
}

extern "C" int rtgl_robust_adaptive_frame(rtgl_context *ctx)
{
    ENTER(ctx);
    RCCHK(masked_frame_refused(ctx, ctx->ra, "rtgl_robust_adaptive_frame", kNoRobustAdaptiveSession, "rtgl_robust_adaptive_frame: rtgl_set_frame_params has not been called"));
    if (ctx->ra.blocks.empty()) return RTGL_OK;
    RCCHK(masked_frame(ctx, ctx->ra.d_samples, ctx->ra.d_lists, (uint32_t)ctx->ra.blocks.size() * 64u));
    RCCHK(robust_adaptive_fold(ctx, ctx->ra.d_samples));
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    return RTGL_OK;
}

extern "C" int rtgl_robust_adaptive_accumulate(rtgl_context *ctx)
{
    ENTER(ctx);
    if (!ctx->ra.active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_adaptive_accumulate") + kNoRobustAdaptiveSession);
    return robust_adaptive_fold(ctx, ctx->d_image);
}

extern "C" int rtgl_robust_adaptive_update(rtgl_context *ctx, rtgl_adaptive_summary *summary_out)
{
    ENTER(ctx);
    if (!summary_out) return fail(ctx, RTGL_ERR_INVALID, "rtgl_robust_adaptive_update: summary_out is NULL");
    if (!ctx->ra.active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_adaptive_update") + kNoRobustAdaptiveSession);
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    TileBucketsEstimateArgs a{};
    a.buckets = ctx->d_ra_buckets; a.records = ctx->ra.d_records; a.n = ctx->ra.d_counts; a.m = ctx->ra.d_counts + (size_t)sh.tx * sh.ty;
    a.plane = rt_robust_tiles_plan::plane_pixels(ctx->width, ctx->height);
    a.width = ctx->width; a.fw = sh.fw; a.fh = sh.fh;
    a.gain = ctx->ra_params.gain; a.floor_ = ctx->ra_params.floor; a.threshold = ctx->ra_params.threshold;
    const dim3 grid((unsigned)sh.tx, (unsigned)sh.ty);
    with_buckets(ctx->ra_K, [&](auto K) { hipLaunchKernelGGL(tile_buckets_estimate_kernel<K>, grid, dim3(256), 0, ctx->stream, a); });
    HIPCHK(ctx, hipGetLastError());
    return tile_session_update(ctx, ctx->ra, ctx->ra_params.min_samples, ctx->ra_params.max_samples, summary_out);
}

extern "C" int rtgl_robust_adaptive_set_mask(rtgl_context *ctx, const uint8_t *tiles)
{
    ENTER(ctx);
    return tile_session_set_mask(ctx, ctx->ra, "rtgl_robust_adaptive_set_mask", kNoRobustAdaptiveSession, tiles);
}

extern "C" int rtgl_robust_adaptive_get_mask(rtgl_context *ctx, uint8_t *tiles)
{
    ENTER(ctx);
    return tile_session_get_mask(ctx, ctx->ra, "rtgl_robust_adaptive_get_mask", kNoRobustAdaptiveSession, tiles);
}

extern "C" int rtgl_robust_adaptive_resolve(rtgl_context *ctx, const rtgl_robust_resolve_params *params)
{
    ENTER(ctx);
    if (!params) return fail(ctx, RTGL_ERR_INVALID, "rtgl_robust_adaptive_resolve: params is NULL");
    rt_robust_plan::ResolveParams P;
    memcpy(&P, params, sizeof P);
    if (const char *why = rt_robust_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_robust_adaptive_resolve: ") + why);
    if (!ctx->ra.active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_adaptive_resolve") + kNoRobustAdaptiveSession);
    const bool to_image = P.dest == rt_robust_plan::kDestImage;
    if (to_image) {                                       // on the host, what rtgl_robust_resolve with dest IMAGE does
        rt_error_plan::drop(ctx->err);                    // (rtgl_error_estimate: another image, the snapshot is dropped)
        ctx->ad.active = false;                           // (adaptive sampling: ... and the session ends)
    }
    const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(ctx->width, ctx->height);
    TileBucketsResolveArgs a{};
    a.buckets = ctx->d_ra_buckets; a.out = to_image ? ctx->d_image : ctx->d_ra_out;
    a.plane = rt_robust_tiles_plan::plane_pixels(ctx->width, ctx->height); a.n = ctx->ra.d_counts;
    a.width = ctx->width; a.height = ctx->height; a.fw = sh.fw; a.fh = sh.fh; a.gain = P.gain;
    const dim3 grid((unsigned)sh.tx, (unsigned)sh.ty);
    with_buckets(ctx->ra_K, [&](auto K) {
        if (to_image) hipLaunchKernelGGL((tile_buckets_resolve_kernel<K, 1>), grid, dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL((tile_buckets_resolve_kernel<K, 0>), grid, dim3(256), 0, ctx->stream, a);
    });
    HIPCHK(ctx, hipGetLastError());
    if (!to_image) ctx->ra_resolved = true;
    return RTGL_OK;
}

extern "C" int rtgl_robust_adaptive_end(rtgl_context *ctx)
{
    ENTER(ctx);
    if (!ctx->ra.active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_adaptive_end") + kNoRobustAdaptiveSession);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // (frames, folds and resolves in flight use the buffers)
    ctx->ra.active = false; ctx->ra_resolved = false; ctx->ra_K = 0;
    ctx->ra.mask.clear(); ctx->ra.blocks.clear(); ctx->ra.tiles.clear();
    return buf_release(ctx, ctx->d_ra_buckets, ctx->ra.d_samples, ctx->d_ra_out, ctx->ra.d_records, ctx->ra.d_counts, ctx->ra.d_lists);
}

extern "C" int rtgl_read_robust_adaptive_f32(rtgl_context *ctx, float *rgba)
{
    ENTER(ctx);
    if (!rgba) return fail(ctx, RTGL_ERR_INVALID, "rtgl_read_robust_adaptive_f32: rgba is NULL");
    if (!ctx->ra.active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_read_robust_adaptive_f32") + kNoRobustAdaptiveSession);
    if (!ctx->ra_resolved) return fail(ctx, RTGL_ERR_STATE, "rtgl_read_robust_adaptive_f32: no rtgl_robust_adaptive_resolve with dest RTGL_ROBUST_DEST_BUFFER since rtgl_robust_adaptive_begin");
    return read_rows(ctx, rgba, ctx->d_ra_out, 16);
}

extern "C" int rtgl_read_robust_adaptive_bucket_f32(rtgl_context *ctx, uint32_t bucket, float *rgba)
{
    ENTER(ctx);
    if (!rgba) return fail(ctx, RTGL_ERR_INVALID, "rtgl_read_robust_adaptive_bucket_f32: rgba is NULL");
    if (!ctx->ra.active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_read_robust_adaptive_bucket_f32") + kNoRobustAdaptiveSession);
    if (bucket >= ctx->ra_K) return fail(ctx, RTGL_ERR_INVALID, "rtgl_read_robust_adaptive_bucket_f32: bucket >= buckets");
    return read_rows(ctx, rgba, ctx->d_ra_buckets + (size_t)bucket * rt_robust_tiles_plan::plane_pixels(ctx->width, ctx->height), 16);
}

extern "C" int rtgl_read_robust_adaptive_tiles(rtgl_context *ctx, rtgl_adaptive_tile *tiles, uint32_t *tx, uint32_t *ty)
{
    ENTER(ctx);
    if (!tiles) return fail(ctx, RTGL_ERR_INVALID, "rtgl_read_robust_adaptive_tiles: tiles is NULL");
    if (!ctx->ra.active) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_read_robust_adaptive_tiles") + kNoRobustAdaptiveSession);
    return tile_session_read_tiles(ctx, ctx->ra, tiles, tx, ty);
}

extern "C" void *rtgl_device_robust_adaptive_tiles(rtgl_context *ctx)
{
    return ctx ? device_plane(ctx, ctx->ra.active, ctx->ra.d_records, "rtgl_device_robust_adaptive_tiles", kNoRobustAdaptiveSession) : nullptr;
}

// ---- rtgl_robust_denoise: the session's resolve and the guided filter in one call (rt_bucket_guide.hpp, rt_bucket_guide_plan.hpp) -------------
static_assert(sizeof(rtgl_robust_denoise_params) == sizeof(rt_bucket_guide_plan::Params) && offsetof(rtgl_robust_denoise_params, gain) == offsetof(rt_bucket_guide_plan::Params, gain)
              && offsetof(rtgl_robust_denoise_params, flags) == offsetof(rt_bucket_guide_plan::Params, flags) && rt_bucket_guide_plan::kFlagDemodulate == (uint32_t)RTGL_DENOISE_DEMODULATE
              && rt_bucket_guide_plan::kPlaneAlbedo == (uint32_t)RTGL_AOV_ALBEDO && rt_bucket_guide_plan::kPlaneNormal == (uint32_t)RTGL_AOV_NORMAL
              && rt_bucket_guide_plan::kPlanePosition == (uint32_t)RTGL_AOV_POSITION && rt_bucket_guide_plan::kLdsBytes == 6u * kBgN * sizeof(float)
              && rt_bucket_guide_plan::kHaloW == (uint32_t)kBgW && rt_bucket_guide_plan::kHaloH == (uint32_t)kBgH, "the layouts of the header and of the kernel");

extern "C" int rtgl_robust_denoise_defaults(rtgl_robust_denoise_params *out)
{
    if (!out) return RTGL_ERR_INVALID;
    const rt_bucket_guide_plan::Params p = rt_bucket_guide_plan::default_params();
    memcpy(out, &p, sizeof p);
    return RTGL_OK;
}

extern "C" int rtgl_robust_denoise(rtgl_context *ctx, const rtgl_robust_denoise_params *params)
{
    ENTER(ctx);
    rt_bucket_guide_plan::Params P = rt_bucket_guide_plan::default_params();
    if (params) memcpy(&P, params, sizeof P);
    if (const char *why = rt_bucket_guide_plan::invalid(P)) return fail(ctx, RTGL_ERR_INVALID, std::string("rtgl_robust_denoise: ") + why);
    if (!ctx->parts.empty() || ctx->world > 1)
        return fail(ctx, RTGL_ERR_STATE, "rtgl_robust_denoise: a tiled or multi-device context holds strips that lack their neighbours' rows; filtering a gathered image is out of scope: "
                                         "render on a single-device context");
    if (const char *why = rt_bucket_guide_plan::refused(ctx->rb_active, ctx->rb_N, ctx->rb_K)) return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_denoise: ") + why);
    if (const char *why = rt_bucket_guide_plan::planes_refused(rt_bucket_guide_plan::planes_needed(P), (uint32_t)ctx->opt.aov, ctx->aov_restart, ctx->aov_n))
        return fail(ctx, RTGL_ERR_STATE, std::string("rtgl_robust_denoise: ") + why);
    const size_t n = rt_bucket_guide_plan::pixels(ctx->local_rows, ctx->width);
    if (n == 0) return fail(ctx, RTGL_ERR_STATE, "rtgl_robust_denoise: this context holds no pixels");
    const bool demod = rt_bucket_guide_plan::demodulates(P), use_n = P.sigma_normal > 0.0f, use_p = P.sigma_position > 0.0f;
    // the prepare kernel writes scratch 0 (passes = 0: the denoised buffer) and, for the last pass's alpha, the resolved pixel into the
    // denoised buffer; pass k reads scratch k & 1 and writes scratch (k + 1) & 1 or, as the last, the denoised buffer: rtgl_denoise_guided's turns
    RCCHK(buf_ensure(ctx, ctx->d_denoised, rt_bucket_guide_plan::record_bytes(n)));
    RCCHK(buf_ensure(ctx, ctx->d_dn_variance, rt_bucket_guide_plan::record_bytes(n)));
    RCCHK(buf_ensure(ctx, ctx->d_dn_near, rt_bucket_guide_plan::near_bytes(n)));
    for (uint32_t k = 0; k < rt_bucket_guide_plan::scratch_buffers(P.passes); ++k) RCCHK(buf_ensure(ctx, ctx->d_dn_scratch[k], rt_bucket_guide_plan::record_bytes(n)));
    BucketGuideArgs b{};
    b.buckets = ctx->d_rb_buckets; b.plane = rt_robust_plan::plane_pixels(ctx->local_rows, ctx->width);
    b.albedo = demod ? ctx->d_aov[0] : nullptr; b.normal = use_n ? ctx->d_aov[1] : nullptr; b.position = use_p ? ctx->d_aov[2] : nullptr;
    b.dst = P.passes == 0u ? ctx->d_denoised : ctx->d_dn_scratch[0]; b.resolved = ctx->d_denoised;
    b.variance = ctx->d_dn_variance; b.near = ctx->d_dn_near;
    b.width = ctx->width; b.height = ctx->local_rows; b.frames = ctx->rb_N; b.gain = P.gain;
    b.inv_normal = use_n ? 1.0f / (P.sigma_normal * P.sigma_normal) : 0.0f;
    b.sigma_position = P.sigma_position;
    b.use_normal = use_n; b.use_position = use_p; b.final_image = P.passes == 0u;
    const dim3 grid(rt_bucket_guide_plan::tiles_x(b.width), rt_bucket_guide_plan::tiles_y(b.height));
    with_buckets(ctx->rb_K, [&](auto K) {
        if (demod) hipLaunchKernelGGL((bucket_guide_kernel<K, true>), grid, dim3(256), 0, ctx->stream, b);
        else hipLaunchKernelGGL((bucket_guide_kernel<K, false>), grid, dim3(256), 0, ctx->stream, b);
    });
    HIPCHK(ctx, hipGetLastError());
    GuidedArgs a{};
    a.image = ctx->d_denoised;                            // (the last pass reads only its own pixel's alpha there, before it writes that pixel)
    a.variance = ctx->d_dn_variance; a.near = ctx->d_dn_near;
    a.albedo = b.albedo; a.normal = b.normal; a.position = b.position;
    a.width = b.width; a.height = b.height;
    a.lum2 = P.sigma_lum * P.sigma_lum;
    a.inv_normal = b.inv_normal; a.sigma_position = P.sigma_position;
    a.use_normal = use_n; a.use_position = use_p; a.demodulate = demod;
    return launch_guided_passes(ctx, a, P.passes, demod);
}

// Keys, ranges and messages: the table of rt_options.hpp.  Here: what an option means to the rest of the context
extern "C" int rtgl_set_option(rtgl_context *ctx, const char *key, int value)
{
    using rt_options::Options;
    ENTER(ctx);
    FANOUT(ctx, rtgl_set_option(part, key, value));
    if (!key) return fail(ctx, RTGL_ERR_INVALID, "key is NULL");
    const rt_options::Row *row = rt_options::find(key);
    if (!row || !(row->flags & rt_options::kSet)) return fail(ctx, RTGL_ERR_INVALID, std::string("unknown option ") + key);
    if (row->field == &Options::kernel_timing) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // (before the value is judged)
    const int before = ctx->opt.*row->field;
    const char *refused = row->field == &Options::aov ? rt_options::refusal(*row, value) : rt_options::set(ctx->opt, *row, value);
    if (refused) return fail(ctx, RTGL_ERR_INVALID, refused);
    if (row->field == &Options::aov) return set_aov(ctx, value);      // stores the mask itself, once the planes are there
    if (row->field == &Options::kernel) ctx->kernel_explicit = true;
    else if (row->field == &Options::mf_group_quads) { ctx->group_explicit = true; if (value != (int)ctx->mf_group_quads) ctx->tris_dirty = true; }      // local origins and A tiles are per group
    else if (row->field == &Options::temporal_moments && value != before) ctx->tm_valid = false;       // moments and colour history always have the same age
    else if (row->field == &Options::kernel_timing) { ctx->kev_used = 0; ctx->kev_frame_start.clear(); ctx->timing_frame_counter = 0; ctx->timing_this_frame = false; }
    return RTGL_OK;
}

extern "C" int rtgl_get_option(rtgl_context *ctx, const char *key, int *value)
{
    ENTER(ctx);
    if (!key || !value) return fail(ctx, RTGL_ERR_INVALID, "NULL argument");
    if (!ctx->parts.empty()) { const int rc = rtgl_get_option(ctx->parts[0], key, value); return rc ? fail(ctx, rc, ctx->parts[0]->error) : RTGL_OK; }
    // read-only keys: what the context did or holds, not what it was asked for
    const struct { const char *key; int value; } derived[] = {
        {"kernel_in_use", ctx->kernel_in_use},                                  // the variant the last frame ran
        {"mf_sets", kSoloSets},
        {"mf_group_quads", (int)ctx->mf_group_quads},                           // the value in use, not the option
        {"camera_lean_frames", (int)ctx->camera_lean_frames},                   // frames of this context that took the lean camera bounce
        {"shade_pass_launches", (int)ctx->shade_pass_launches},                 // launches of this context that took the one-pass shade_kernel
        {"cand_region_pairs", (int)ctx->cand_region_pairs},                     // kernel 4: current capacity of one wave's candidate region
        {"device_mbytes", (int)((ctx->buffers.total_bytes() + (1u << 20) - 1) >> 20)},      // device memory held by this context: the ledger's sum (MiB, rounded up)
    };
    for (const auto &d : derived) if (!strcmp(d.key, key)) { *value = d.value; return RTGL_OK; }
    const rt_options::Row *row = rt_options::find(key);
    if (!row || !(row->flags & rt_options::kGet)) return fail(ctx, RTGL_ERR_INVALID, std::string("unknown option ") + key);
    *value = ctx->opt.*row->field;
    return RTGL_OK;
}

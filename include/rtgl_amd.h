/*
 * rtgl_amd.h -- C ABI of the MI355X-native progressive path tracer (drop-in boundary).
 *
 * The reference (gue-ni/raytracer.glsl) has no plugin / FFI layer: its hot path sits behind the
 * C++ class `Renderer : public Window` (reference src/renderer.h:127-148) and the OpenGL driver.
 * This header is the flat C boundary a maintainer binds instead of the GL calls; the C++ facade
 * in include/rtgl/renderer.h (same class names and method signatures as the reference) is a thin
 * layer over exactly these entry points.  Each entry point cites the reference interface it
 * replaces.  Plain pointers and sizes only; every call returns 0 on success or a negative
 * rtgl_status, with text available from rtgl_last_error().
 *
 * Threading (reference: single-threaded, everything on the thread that owns the GL context,
 * src/window.cpp:13): one host thread per context; calls on one context must not overlap.
 * Ownership (reference: setters copy synchronously via glBufferData, src/gfx/gl.h:93-97): every
 * upload copies; the caller may free its buffer as soon as the call returns.
 */
#ifndef RTGL_AMD_H
#define RTGL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtgl_context rtgl_context;

typedef enum rtgl_status {
    RTGL_OK = 0,
    RTGL_ERR_INVALID = -1,   /* bad argument */
    RTGL_ERR_DEVICE = -2,    /* HIP runtime error (text in rtgl_last_error) */
    RTGL_ERR_NO_DEVICE = -3, /* no usable gfx950 device: the library has no CPU fallback */
    RTGL_ERR_STATE = -4      /* call not valid in the current state */
} rtgl_status;
/* Order of the checks: a call that is wrong in its arguments AND in the state of the context reports the arguments (RTGL_ERR_INVALID): every
 * entry point checks its parameters before it looks at the context.  Two checks need the context and come after its state: n < 1 of
 * rtgl_error_estimate (F_n is known only once a frame has been rendered) and samples / max_bounce of rtgl_adaptive_frame and of
 * rtgl_robust_adaptive_frame (a masked frame of either kind without a session or with "aov" on is RTGL_ERR_STATE whatever `samples` is).  A post-process
 * call (rtgl_denoise and everything below it in this header) that is refused changes nothing: no buffer, no option, no session, no snapshot. */

/* The 17 uniforms of reference shaders/raytracer.glsl:62-81, set per frame by
 * src/renderer.cpp:96-123 (glUniform* by name).  camera_fov is in radians (renderer.cpp:116).
 * `time` is uploaded by the reference but never read by the shader; kept for symmetry. */
typedef struct rtgl_frame_params {
    int32_t  frames;       /* u_frames  = Window::m_frames after the pre-render increment (window.cpp:42) */
    uint32_t samples;      /* u_samples (renderer.h:168: always 1 in the reference) */
    uint32_t max_bounce;   /* u_max_bounce */
    float    time;         /* u_time (dead) */
    float    background[3];
    int32_t  reset_flag;   /* u_reset_flag */
    int32_t  use_envmap;   /* u_use_envmap (false when no cube map is set, renderer.cpp:104-110) */
    int32_t  use_dof;      /* u_use_dof */
    int32_t  random;       /* u_random = rand() once per frame (renderer.cpp:102) */
    float    camera_position[3];
    float    camera_fov;
    float    camera_aperture;
    float    camera_focal_length;
    float    camera_forward[3];
    float    camera_up[3];
    float    camera_right[3];
} rtgl_frame_params;

/* Device-side work counters of the last rendered frame (no reference counterpart; feeds the
 * Msegments/s and Gtests/s figures of SURVEY.md 8(d1)). */
typedef struct rtgl_counters {
    uint64_t paths;          /* pixel-samples started */
    uint64_t segments;       /* bounce iterations executed */
    uint64_t triangle_tests; /* ray x triangle edge-function evaluations */
    uint64_t candidates;     /* tests that reached the exact (reference-order) re-evaluation */
    uint64_t env_lookups;
    uint64_t culled_tests;   /* of triangle_tests: pairs skipped by the packet cull (certified rejections, never evaluated) */
    uint64_t reserved[2];
} rtgl_counters;

/* Kernel variants (rtgl_set_option "kernel"; the environment variable RTGL_AMD_KERNEL=0, 1, 2 or 4 changes the default of new
 * contexts).  All produce bit-identical images.  Unless a variant was requested explicitly, a scene without triangles is rendered
 * with RTGL_KERNEL_MEGA (there is no scan to split off; one launch per frame). */
enum {
    RTGL_KERNEL_MEGA = 0,            /* one launch per frame, one lane per pixel, whole path in registers */
    RTGL_KERNEL_WAVEFRONT = 1,       /* one fused launch per bounce over the compacted ray queue */
    RTGL_KERNEL_WAVEFRONT_SPLIT = 2, /* per bounce: intersect (ray blocks x triangle chunks, fp32 VALU filter) + shade */
    RTGL_KERNEL_REMOVED_3 = 3,       /* (round 1's three-waves-per-SIMD matrix-core scan: not deterministic, removed; refused) */
    RTGL_KERNEL_WAVEFRONT_MFMA_SOLO = 4 /* default: as 2, with a conservative bf16 matrix-core broad phase in front of the exact test: one or two
                                         * waves per SIMD, persistent blocks, A tiles in LDS, hand-ordered instruction stream, exact tests in a
                                         * separate narrow-phase kernel */
};

/* First-hit auxiliary planes (option "aov" = a mask of the bits below; no reference counterpart).  Per local pixel one 16-byte record per
 * enabled plane, laid out like the image (rows bottom-up; a tiled context holds its local strips, packed like the image):
 *   RTGL_AOV_ALBEDO    float4  hit: albedo of the hit material exactly as the shader loads it, a = 1.  Miss: the background colour, or the
 *                              cube-map value the camera ray received when u_use_envmap is on, a = 0.
 *   RTGL_AOV_NORMAL    float4  hit: the normal shading uses (sphere: (p - c) / r; triangle: its stored plane normal), not flipped for
 *                              inside hits, w = 0.  Miss: 0.
 *   RTGL_AOV_POSITION  float4  hit: the hit point shading uses (o + d t), w = t.  Miss: 0.
 *   RTGL_AOV_IDS       int32x4 {kind, object, primitive, material}: kind 1 sphere (object = primitive = sphere index), kind 2 triangle (object =
 *                              mesh index, primitive = the triangle's index in the vertex buffer, vertex / 3).  Miss: {0, -1, -1, -1}.
 * The first hit is the camera ray's hit at bounce 0, chosen exactly as shading chooses it (a mesh wins a tie with a sphere; among
 * triangles the lowest visit index, which also decides the mesh of a triangle listed by two meshes).  With u_samples > 1 every sample
 * reuses the camera ray: the planes are written once per frame.  u_max_bounce == 0 traces no ray: the frame contributes a miss with albedo 0.
 * Accumulation: the three float planes hold the mean over the frames since they last restarted, v = (x + prev * (n - 1)) / n in float32
 * (n == 1: v = x exactly), where n restarts at 1 on a frame with u_reset_flag != 0, on the first frame after rtgl_clear_image and on the
 * first frame after "aov" is set, and otherwise counts the frames.  (Not the image's formula, which divides a reset frame by frames + 1.)
 * The ids plane is always the last frame's.  rtgl_write_image_f32 does not touch the planes.  Default 0: no planes, nothing changes.
 * Setting "aov" allocates the enabled planes zeroed (and frees the others); while it is non-zero frames are rendered one by one. */
enum {
    RTGL_AOV_ALBEDO = 1,
    RTGL_AOV_NORMAL = 2,
    RTGL_AOV_POSITION = 4,
    RTGL_AOV_IDS = 8,
    RTGL_AOV_ALL = 15
};

/* -- lifetime: replaces Renderer::Renderer(width,height) GL object creation (src/renderer.cpp:21-64).
 * The accumulation image is RGBA32F, width x height, zero-initialised (the reference leaves it
 * undefined).  device = HIP device ordinal. */
int rtgl_create(rtgl_context **out, int width, int height, int device);

/* Same, but this context owns only the row strips s with (s % world) == rank, where strip s covers
 * image rows [s*strip_rows, (s+1)*strip_rows).  Pixel seeds and camera rays use absolute pixel
 * coordinates, so the union over ranks is bit-identical to a single-context render.  strip_rows
 * must be a multiple of 8.  (No reference counterpart: SURVEY.md 8(e).)  The calls that need the whole picture say below that they are RTGL_ERR_STATE
 * on such a context; rtgl_temporal_reset, rtgl_tonemap_reset and rtgl_error_reset only drop state that such a context never has, and
 * return RTGL_OK. */
int rtgl_create_tiled(rtgl_context **out, int width, int height, int device, int rank, int world, int strip_rows);

/* Single-process multi-device context: the image is cut into strips of strip_rows rows, strip s belongs to
 * devices[s % n_devices]; every device holds the whole scene and renders its strips (one dispatch per device replaces the single
 * glDispatchCompute of src/renderer.cpp:129-134); the tile buffers are gathered to devices[0] (peer copies over xGMI, one 2-D copy
 * per device) when the image is read -- rtgl_read_image_* do it implicitly, rtgl_gather_tiles explicitly (then rtgl_device_image
 * is the assembled image on devices[0]).  Every other entry point takes the handle like a single-device one: uploads and options
 * go to all devices, counters are summed, rtgl_last_frame_ms is the slowest device.  Bit-identical to a single-device render.
 * The same ordinal may appear more than once.  rtgl_bind_device_image / rtgl_set_stream are refused on such a handle.
 * rtgl_render_frame hands each device's frame to a submit thread of the context's own (created here, joined in rtgl_destroy) and returns
 * when all have submitted; the environment variable RTGL_AMD_MULTI_THREADS=0, read here, keeps submission on the caller's thread. */
int rtgl_create_multi(rtgl_context **out, int width, int height, const int *devices, int n_devices, int strip_rows);
int rtgl_device_count(const rtgl_context *ctx);   /* 1 for a single-device context */
int rtgl_gather_tiles(rtgl_context *ctx);         /* enqueue the gather on devices[0]'s stream (no-op for a single-device context); every device's
                                                    * stream then waits for the copies before its next frame (the tiles are being read) */

void rtgl_destroy(rtgl_context *ctx);
const char *rtgl_last_error(const rtgl_context *ctx); /* ctx may be NULL: error of the last failed create */

/* -- scene upload: replaces the set_* family (src/renderer.cpp:151-216), layouts per the shader's
 * buffer declarations (shaders/raytracer.glsl:11-60).  count = number of elements. */
int rtgl_upload_spheres(rtgl_context *ctx, const void *spheres, uint32_t count);     /* 32 B each; set_spheres :151-155 */
int rtgl_upload_materials(rtgl_context *ctx, const void *materials, uint32_t count); /* 32 B each; set_materials :157-161 */
int rtgl_upload_meshes(rtgl_context *ctx, const void *meshes, uint32_t count);       /* 16 B each; set_meshes :181-185 */
int rtgl_upload_vertices(rtgl_context *ctx, const void *vec4s, uint32_t vec4_count); /* 16 B each, 3 per triangle; set_vertices :174-179 */
int rtgl_upload_nodes(rtgl_context *ctx, const void *nodes, uint32_t count);         /* 48 B each; set_nodes :187-191 */
/* A node's spheres are the indices offset <= i < offset + count with the sum taken in 32-bit unsigned arithmetic, as the shader takes it
 * (:305): a sum that wraps below offset names no sphere, an index past the sphere buffer names the all-zero sphere.  A buffer whose walk
 * makes more than 2^20 sphere tests per ray is refused by the next rtgl_render_frame (RTGL_ERR_INVALID). */
/* faces: 6 (or fewer) tightly packed 8-bit images in +X,-X,+Y,-Y,+Z,-Z order, channels 3 or 4;
 * replaces CubemapTexture's constructor (src/gfx/gl.cpp:241-260) + set_envmap (renderer.cpp:163-172).
 * nfaces < 6 reproduces the incomplete cube of a failed face load (lookups return black). */
int rtgl_upload_envmap(rtgl_context *ctx, const uint8_t *faces, int nfaces, int width, int height, int channels);

/* -- per frame: replaces the uniform uploads + glDispatchCompute + glMemoryBarrier of
 * Renderer::render (src/renderer.cpp:96-134).  rtgl_render_frame enqueues on the context's stream
 * and returns; rtgl_synchronize waits.  (Option "frame_batch" > 1: it may hold the frame back until the batch is full, see below.) */
int rtgl_set_frame_params(rtgl_context *ctx, const rtgl_frame_params *params);
int rtgl_render_frame(rtgl_context *ctx);
int rtgl_synchronize(rtgl_context *ctx);

/* -- image access: replaces glGetTexImage in save_to_file (src/renderer.cpp:218-223).
 * f32: RGBA32F rows bottom-up exactly as stored (row 0 = pixel y 0).  For a tiled context the
 * buffer holds only the local strips, packed in increasing strip order (rtgl_local_rows rows).
 * u8: clamp to [0,1], scale by 255, round to nearest (what GL_UNSIGNED_BYTE readback does);
 * flip != 0 writes the top row first like stbi_write_png's flipped output (renderer.cpp:240). */
int rtgl_read_image_f32(rtgl_context *ctx, float *rgba);
int rtgl_read_image_u8(rtgl_context *ctx, uint8_t *rgba, int flip);
int rtgl_write_image_f32(rtgl_context *ctx, const float *rgba); /* preload / resume the accumulation image */
int rtgl_clear_image(rtgl_context *ctx);
int rtgl_local_rows(const rtgl_context *ctx);      /* rows held by this context (== height when not tiled) */
int rtgl_local_row_to_global(const rtgl_context *ctx, int local_row);

/* -- plumbing for callers that own device memory / streams (PyTorch, RCCL) */
void *rtgl_device_image(rtgl_context *ctx);                 /* device pointer of the local RGBA32F buffer (NULL: see rtgl_last_error) */
int rtgl_bind_device_image(rtgl_context *ctx, void *dptr);  /* render into caller-owned device memory (local_rows*width*16 B) */
/* hipStream_t; NULL restores the context's own stream.  All contexts of a process on one device submit to ONE stream of the library's by
 * default, so that their pipelines never run concurrently (several path-tracing pipelines at once on one MI355X have produced wrong
 * frames: DESIGN.md 5.2).  rtgl_set_stream therefore FAILS with RTGL_ERR_STATE when another live context of the process renders on a
 * different stream of the same device; bind the same stream to all of them, or set RTGL_AMD_ALLOW_CONCURRENT_PIPELINES=1 and take the
 * ordering over.  The library cannot see other PROCESSES on the device: do not run two path-tracing processes on one GPU at the same time.
 * With "frame_batch" > 1, synchronising the bound stream is NOT enough to know that a frame has been submitted: only rtgl_synchronize and
 * the read-out calls submit the frames a batching context holds back. */
int rtgl_set_stream(rtgl_context *ctx, void *hip_stream);

/* -- diagnostics */
int rtgl_get_counters(rtgl_context *ctx, rtgl_counters *out);  /* synchronises */
int rtgl_read_rng_state(rtgl_context *ctx, uint32_t *xyzw);    /* per local pixel final PCG4D state of the last frame; needs option "rng_state"=1 */

/* -- first-hit planes (option "aov", above).  plane = ONE RTGL_AOV_* bit.  rtgl_read_aov copies local_rows x width x 16 bytes (a multi-device
 * handle: the whole image's rows, assembled on the host); RTGL_ERR_STATE when the plane is not enabled, RTGL_ERR_INVALID for a bad plane or
 * a NULL pointer.  rtgl_device_aov: the plane's device pointer (torch interop); NULL on a multi-device handle or for a plane that is not
 * enabled, see rtgl_last_error.  The pointer stays valid until "aov" is set again or the context is destroyed. */
int rtgl_read_aov(rtgl_context *ctx, int plane, void *out);
void *rtgl_device_aov(rtgl_context *ctx, int plane);

/* -- guide pass: the first-hit planes without a frame.  rtgl_guides_frame traces, for every pixel of the dispatch footprint, the camera ray
 * of sample 0 that rtgl_render_frame would draw from the current frame parameters, and folds its first hit into the enabled planes.
 *   The ray.  Camera, random, depth of field, background and environment come from rtgl_set_frame_params; frames, reset_flag, samples and
 *   max_bounce are ignored, and the ray is traced even with max_bounce == 0 (where a frame contributes a miss with albedo 0).
 *   The hit is chosen exactly as bounce 0 of shading chooses it (a mesh wins a tie with a sphere; among triangles the lowest visit index);
 *   a miss records the background or the cube-map value.  The records are those of the planes above, bit for bit what a frame of the same
 *   parameters writes, whatever option "kernel" says: a scene without triangles takes one launch, a scene with triangles the lean ray
 *   generation, the intersect stage of bounce 0 (kernel 2's for "kernel" = 2, otherwise kernel 4's with fresh keep bits) and that launch.
 *   The fold is the planes' own: n = 1 if a restart is pending (after rtgl_clear_image, after "aov" is set, after
 *   rtgl_adaptive_begin), otherwise n + 1; v = (x + prev * (n - 1)) / n in float32, n == 1 stores x exactly; the ids plane
 *   holds this pass's ids.  The pass clears the pending restart and counts as a frame since the planes restarted for every call that asks
 *   for one (rtgl_denoise, rtgl_denoise_guided, rtgl_robust_denoise, rtgl_temporal_accumulate, rtgl_temporal_clip); a later rtgl_render_frame
 *   without reset_flag continues the same n.
 *   Nothing else is written: not the image, the sample and bucket buffers, the RNG states, the counters, the denoised, temporal and display
 *   buffers, nor the snapshot of rtgl_error_estimate, and the pass ends no session -- adaptive, robust and robust adaptive sessions stay open,
 *   so masked frames (which write no planes) and the denoisers can be combined, and the guides of a session can be averaged.  The ray counts
 *   the frame path sizes its grids by stay as they are, and the kept camera bits are neither taken nor dropped: every later frame is
 *   bit-identical to the frame of a context that never made the call.  rtgl_last_frame_ms covers the pass.
 * Frames a batching context holds are submitted first; the call enqueues on the context's stream and returns.  A tiled context works on its
 * own strips.  An empty footprint (an image below 8 x 8) enqueues nothing, returns RTGL_OK and counts as a pass, as a frame does.
 * RTGL_ERR_INVALID: ctx is NULL.  RTGL_ERR_STATE, in this order: a multi-device handle; no frame parameters; option "aov" is 0.  A refused
 * call moves neither the planes nor n. */
int rtgl_guides_frame(rtgl_context *ctx);

/* -- denoiser: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the accumulation image, guided by the first-hit planes,
 * with albedo demodulation and the compact polynomial (1 - x/4)^4 in place of exp(-x).  No reference counterpart.  What a caller of a
 * 1-spp progressive renderer needs for a usable picture after a handful of frames.  The filter uses only + - x / and compares, so it is
 * DEFINED bit for bit (tests/denoise_mirror.py restates it in numpy): all arithmetic binary32, one rounding per operation, in exactly the
 * order written here, no contraction, correctly rounded divide.
 *   Inputs: the image I (RGBA32F) and the planes A (albedo), N (normal), P (position, w = t) as they are on the context's stream when the
 *   call is enqueued, over all width x height pixels.
 *   ew(x):  q = (x < 4) ? 1 - 0.25 x : 0;  q = q q;  q = q q;  ew = q   (a NaN x gives 0).      dot3(v) = (v.x v.x + v.y v.y) + v.z v.z.
 *   h = [1/16, 1/4, 3/8, 1/4, 1/16].
 *   Demodulation: per channel d = (A > 2^-10) ? A : 2^-10;  c0 = I.rgb / d when RTGL_DENOISE_DEMODULATE is set, else c0 = I.rgb.
 *   Pass L = 0 .. passes-1, step s = 2^L, per pixel p, c the previous pass's output:
 *     sig = sigma_color 2^-L;  ic = 1 / (sig sig);  in = 1 / (sigma_normal sigma_normal);  sp = sigma_position P(p).w;
 *     ip = (sp > 0) ? 1 / (sp sp) : 0      (the position tolerance grows with the hit distance; on a miss, t = 0, the factor sees x = 0 and the
 *                                           normal term separates hit from miss)
 *     taps j = -2..2 (rows, outer), i = -2..2 (inner), q = p + (i s, j s); a tap outside the image is skipped:
 *       w = h[j] h[i];  w = w ew(dot3(c(q) - c(p)) ic);  w = w ew(dot3(N(q).xyz - N(p).xyz) in);  w = w ew(dot3(P(q).xyz - P(p).xyz) ip)
 *       (a term whose sigma is <= 0 is switched off: its factor is skipped and its plane never read)
 *       only if w > 0:  acc = acc + w c(q) per channel,  ws = ws + w
 *     c'(p) = (ws > 0) ? acc / ws : c(p)
 *   Result: rgb = demodulating ? c d : c,  a = I.a.  passes = 0 without demodulation is the identity, bit for bit.
 * Defaults (rtgl_denoise_defaults, and a NULL params): passes 5, sigma_color 16, sigma_normal 0.3, sigma_position 0.05, demodulate on.
 * rtgl_denoise first submits the frames a batching context holds, then enqueues passes kernels on the context's stream and returns without
 * waiting.  It writes the context's DENOISED buffer (and two scratch buffers; all three allocated by the first call that needs them, freed
 * with the context) and nothing else: image, planes, RNG states and counters are only read.  The denoised buffer is a snapshot: later
 * frames do not change or invalidate it; the next rtgl_denoise overwrites it.
 * RTGL_ERR_INVALID: NULL context, passes > 8, a non-finite sigma, unknown flag bits, non-zero reserved.  RTGL_ERR_STATE: a plane the
 * parameters need is not enabled (option "aov": A iff demodulating, N iff sigma_normal > 0, P iff sigma_position > 0); a plane is needed
 * and no frame has been rendered since the planes last restarted; the context is tiled or multi-device (a strip lacks its neighbours'
 * rows; filtering a gathered image is out of scope).  rtgl_read_denoised_f32 (synchronises; layout of rtgl_read_image_f32) and
 * rtgl_device_denoised (torch interop; valid until the context is destroyed) return RTGL_ERR_STATE / NULL before the first successful
 * rtgl_denoise. */
enum { RTGL_DENOISE_DEMODULATE = 1 };
typedef struct rtgl_denoise_params {
    uint32_t passes;          /* 0..8 */
    float    sigma_color;     /* <= 0: the colour term is off */
    float    sigma_normal;    /* <= 0: the normal term is off */
    float    sigma_position;  /* <= 0: the position term is off; relative to the hit distance */
    uint32_t flags;           /* RTGL_DENOISE_DEMODULATE */
    uint32_t reserved[3];     /* must be 0 */
} rtgl_denoise_params;        /* 32 bytes */
int rtgl_denoise_defaults(rtgl_denoise_params *out);
int rtgl_denoise(rtgl_context *ctx, const rtgl_denoise_params *params);
int rtgl_read_denoised_f32(rtgl_context *ctx, float *rgba);
void *rtgl_device_denoised(rtgl_context *ctx);

/* -- variance-guided denoiser: the filter above with the global colour tolerance replaced by a luminance tolerance that follows a per-pixel
 * variance estimate (after SVGF, Schied et al. 2017, spatial part only), the estimate filtered along with the colour, and a firefly clamp
 * in front.  A call of its own beside rtgl_denoise; it reads the same inputs and writes the same DENOISED buffer.  DEFINED bit for bit under
 * the same rules (tests/denoise_guided_mirror.py restates it): binary32, only + - x / compares and selects, one rounding per operation in
 * the order written, no contraction, correctly rounded divide, rows outer and columns inner, a tap outside the image is skipped.
 *   ew, dot3, h, d, c0, in, ip and the normal and position factors: as above.     lum(c) = (0.25 c.r + 0.5 c.g) + 0.25 c.b.
 *   Geometric weight of a tap q of p:  g(q) = 1;  g = g ew(dot3(N(q).xyz - N(p).xyz) in);  g = g ew(dot3(P(q).xyz - P(p).xyz) ip), ip from
 *     P(p).w  (a term whose sigma is <= 0 is skipped).  A neighbour q = p + (i, j), |i|, |j| <= 1, is NEAR p if it is inside the image and
 *     g(q) > 0: the clamp and the variance blur below look at near neighbours only, so that nothing reaches p across an edge of the guides.
 *   Firefly clamp (firefly_ratio > 0), per pixel p: over its up to 8 near neighbours q = p + (i, j), j = -1..1 (outer), i = -1..1,
 *     (i, j) != (0, 0): m = lum(c0(q)) for the first of them, then m = (lum(c0(q)) > m) ? lum(c0(q)) : m  (a NaN never replaces a number).
 *     l = lum(c0(p));  k = firefly_ratio m;  if there is a near neighbour and l > k:  s = k / l,  c1(p) = c0(p) s per channel;  else c1(p) = c0(p).
 *     With the clamp off c1 = c0.
 *   Spatial variance, per pixel p: taps j = -3..3 (outer), i = -3..3, q = p + (i, j), l(q) = lum(c1(q)):
 *       only if g(q) > 0 and l(q) - l(q) == 0 (a finite luminance):  s0 = s0 + g,  s1 = s1 + g l(q),  s2 = s2 + g (l(q) l(q))
 *     if s0 > 0:  mu = s1 / s0;  v = s2 / s0 - mu mu;  v0 = (v > 0) ? v : 0.      else mu = 0, v0 = 0.
 *   Pass L = 0 .. passes-1, step s = 2^L, per pixel p, c and var the previous pass's output (c1 and v0 for the first):
 *     vg = vs / vw over p itself and its near neighbours q = p + (i, j), j = -1..1 (outer), i = -1..1, unit spacing whatever the step,
 *       b = [1/4, 1/2, 1/4]:  w = b[j] b[i];  vs = vs + w var(q),  vw = vw + w
 *     il = 1 / ((sigma_lum sigma_lum) vg + 2^-20)         (sigma_lum is NOT halved from pass to pass: the variance shrinks by itself)
 *     taps j = -2..2 (outer), i = -2..2, q = p + (i s, j s):
 *       dl = lum(c(q)) - lum(c(p));  w = h[j] h[i];  w = w ew((dl dl) il);  then the normal and the position factor as above
 *       only if w > 0:  acc = acc + w c(q) per channel,  ws = ws + w,  va = va + (w w) var(q)
 *     c'(p) = (ws > 0) ? acc / ws : c(p);   var'(p) = (ws > 0) ? va / (ws ws) : var(p)
 *   Result: rgb = demodulating ? c d : c,  a = I.a.  The VARIANCE buffer holds {mu, v0, var after the last pass, s0} per pixel, in the
 *   image's layout (variances of the demodulated luminance when demodulating).  passes = 0 with the clamp off and without demodulation is
 *   the identity, bit for bit.
 * Defaults (rtgl_denoise_guided_defaults, and a NULL params): passes 5, sigma_lum 4, sigma_normal 0.3, sigma_position 0.05, firefly_ratio 1,
 * demodulate on.
 * Like rtgl_denoise it first submits the frames a batching context holds, enqueues on the context's stream and returns without waiting; it
 * writes the denoised buffer (the later of the two calls overwrites the earlier), the two scratch buffers and the variance buffer
 * (allocated by the first call that needs them, freed with the context) and nothing else.
 * RTGL_ERR_INVALID: NULL context, passes > 8, a non-finite sigma or ratio, sigma_lum <= 0, unknown flag bits, non-zero reserved.
 * RTGL_ERR_STATE: exactly the conditions of rtgl_denoise.  rtgl_read_denoise_variance_f32 (synchronises) and rtgl_device_denoise_variance
 * (valid until the context is destroyed) return RTGL_ERR_STATE / NULL before the first successful rtgl_denoise_guided. */
typedef struct rtgl_denoise_guided_params {
    uint32_t passes;          /* 0..8 */
    float    sigma_lum;       /* > 0: luminance tolerance in standard deviations */
    float    sigma_normal;    /* <= 0: the normal term is off */
    float    sigma_position;  /* <= 0: the position term is off; relative to the hit distance */
    float    firefly_ratio;   /* <= 0: clamp off; else a pixel brighter than ratio x its brightest neighbour is scaled down to that */
    uint32_t flags;           /* RTGL_DENOISE_DEMODULATE */
    uint32_t reserved[2];     /* must be 0 */
} rtgl_denoise_guided_params; /* 32 bytes */
int rtgl_denoise_guided_defaults(rtgl_denoise_guided_params *out);
int rtgl_denoise_guided(rtgl_context *ctx, const rtgl_denoise_guided_params *params);
int rtgl_read_denoise_variance_f32(rtgl_context *ctx, float *rgba);
void *rtgl_device_denoise_variance(rtgl_context *ctx);

/* -- temporal accumulation: the accumulated radiance of the previous view reprojected into the current one and blended with the current
 * frame (the temporal half of SVGF, Schied et al. 2017; the spatial half is rtgl_denoise_guided).  No reference counterpart: the reference
 * answers a camera move with u_reset_flag, back to 1 spp.  DEFINED bit for bit under the denoisers' rules (tests/temporal_mirror.py restates
 * it): binary32, only + - x / compares, selects and floor (exact), one rounding per operation in the order written, no contraction,
 * correctly rounded divide.   ew, dot3, in = 1 / (sigma_normal sigma_normal): as in rtgl_denoise.   dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
 *   Inputs, as they are on the context's stream when the call is enqueued: the image I, the planes N and P, the context's current
 *   rtgl_frame_params (the CURRENT camera); and from the previous successful call: its output Hp (rgb, a = n), its copies Np, Pp of the
 *   planes, its camera.  W = width, H = height.
 *   Camera record, built on the host per call: position, forward, up, right;  hw = (float)tan((double)camera_fov * 0.5);
 *     asp = (float)height / (float)width;  wd = 2 hw;  ht = 2 (hw asp);  ff = dot(forward, forward), rr = dot(right, right), uu = dot(up, up);
 *     kx = ff / (wd rr);  ky = ff / (ht uu).   The axes are taken to be mutually orthogonal, as the reference's camera makes them.
 *   Per pixel p = (px, py):
 *     hit = P(p).w > 0.   Hit: v = P(p).xyz - position_prev.   Miss: the pixel's own pinhole direction through the CURRENT camera,
 *       x = ((float)px / (float)W) 2 - 1,  y = ((float)py / (float)H) 2 - 1,  v = (forward + (right wd) x) + (up ht) y per component (the
 *       background is at infinity: translation is ignored).
 *     f = dot(v, forward_prev);  sx = ((((dot(v, right_prev) / f) kx_prev) + 1) 0.5) W;  sy = ((((dot(v, up_prev) / f) ky_prev) + 1) 0.5) H.
 *     There is no history unless f > 0, sx >= -1, sx < W, sy >= -1 and sy < H (a NaN fails).
 *     x0 = floor(sx), fx = sx - x0;  y0 = floor(sy), fy = sy - y0.
 *     Taps q = (x0 + i, y0 + j), j = 0, 1 (outer), i = 0, 1;  b = (i ? fx : 1 - fx) (j ? fy : 1 - fy);  a tap outside the image is skipped.
 *     Static shortcut: when every field of the previous camera record compares equal to the current one's, the four taps are replaced by
 *       the single tap q = p with b = 1: a camera at rest accumulates a plain per-pixel mean, no resampling blur.
 *     A tap counts only if its kind matches: (Pp(q).w > 0) == hit.
 *     Hit:  w = b;  w = w ew(dot3(Np(q).xyz - N(p).xyz) in);  w = w ew(dot3(Pp(q).xyz - P(p).xyz) ip),  sp = sigma_position P(p).w,
 *       ip = (sp > 0) ? 1 / (sp sp) : 0   (a term whose sigma is <= 0 is skipped).     Miss:  w = b.
 *     only if w > 0:  acc = acc + w Hp(q).rgb per channel,  na = na + w Hp(q).a,  ws = ws + w
 *     If there is history and ws > 0:  h = acc / ws;  n = na / ws + 1;  n = (n > max_history) ? max_history : n;  al = 1 / n;
 *       out = h + (I.rgb - h) al per channel.     Else out = I.rgb, n = 1.
 *   Stores: {out, n} to the other history buffer; P(p) and, when the normal plane is enabled (whatever sigma_normal), N(p), as read, to the
 *   other guide copies; the host keeps the camera record.  With sigma_normal <= 0 the normal plane need not be enabled and is then neither
 *   read nor copied.
 *   rtgl_temporal_reset and a change of "temporal_moments" drop the history for the NEXT rtgl_temporal_accumulate only: the latest history
 *   buffer (and its moments) stay what rtgl_read_temporal_f32, "denoise_source" = 1, rtgl_tonemap source 2 and rtgl_temporal_clip work on.
 *   The CURRENT camera is that of the latest rtgl_set_frame_params, whether or not a frame was rendered with it.
 *   The first call and the first after rtgl_temporal_reset have no history (out = I.rgb, n = 1 everywhere).  The history is dropped in the
 *   same way when this call needs Np and the previous call stored none because the normal plane was off then.
 * Defaults (rtgl_temporal_defaults, and a NULL params): max_history 32, sigma_normal 0.3, sigma_position 0.05.
 * Intended use: render each frame with reset_flag = 1, frames = 0, so that the image ((color + 0 x 0) / (0 + 1) = color) and the planes are that
 * frame's own; call rtgl_temporal_accumulate after every frame; read the history, or set option "denoise_source" = 1 and denoise it.
 * Like the denoisers the call first submits the frames a batching context holds, enqueues one kernel on the context's stream and returns
 * without waiting.  It writes only its own buffers (two history buffers, two copies of the position plane and two of the normal plane,
 * allocated by the first call that needs them, freed with the context): image, planes, RNG states, counters, the denoised and the
 * variance buffer are only read.
 * RTGL_ERR_INVALID: NULL context, a non-finite parameter, max_history < 1, non-zero flags or reserved words.  RTGL_ERR_STATE:
 * RTGL_AOV_POSITION is not enabled; RTGL_AOV_NORMAL is not enabled while sigma_normal > 0; no frame has been rendered since the planes last
 * restarted; the context is tiled or multi-device.  rtgl_read_temporal_f32 (synchronises; layout of rtgl_read_image_f32; a = the history
 * length n) and rtgl_device_temporal return RTGL_ERR_STATE / NULL before the first successful rtgl_temporal_accumulate.  The two history
 * buffers take turns: rtgl_device_temporal names the one the LATEST call wrote, so ask again after each call.
 * Option "denoise_source": 0 (default) rtgl_denoise and rtgl_denoise_guided filter the image; 1 they take the latest history buffer wherever
 * they take the image (the result's alpha is then the history length) and return RTGL_ERR_STATE while no rtgl_temporal_accumulate has
 * succeeded; any other value is RTGL_ERR_INVALID.
 * Limits: static scenes only (no motion vectors: re-uploaded geometry is caught by the position test alone); mirrors and glass reproject
 * by their first hit; with depth of field the position is the jittered ray's hit; a NaN radiance stays in a pixel's history until a reset
 * or a disocclusion. */
typedef struct rtgl_temporal_params {
    float    max_history;     /* >= 1: the history length is capped here (the blend factor is never below 1 / max_history) */
    float    sigma_normal;    /* <= 0: the normal test is off (the normal plane is then not needed) */
    float    sigma_position;  /* <= 0: the position test is off; relative to the current hit distance, as in rtgl_denoise */
    uint32_t flags;           /* none defined: must be 0 */
    uint32_t reserved[4];     /* must be 0 */
} rtgl_temporal_params;       /* 32 bytes */
int rtgl_temporal_defaults(rtgl_temporal_params *out);
int rtgl_temporal_accumulate(rtgl_context *ctx, const rtgl_temporal_params *params);
int rtgl_temporal_reset(rtgl_context *ctx);                 /* the next rtgl_temporal_accumulate starts without history */
int rtgl_read_temporal_f32(rtgl_context *ctx, float *rgba);
void *rtgl_device_temporal(rtgl_context *ctx);

/* -- temporal luminance moments: the first and second moment of each frame's luminance carried through the reprojection above with the
 * same taps, weights and blend as the colour, so that rtgl_denoise_guided can be guided by the variance the frames themselves showed
 * instead of one estimated from 49 neighbours of the averaged picture (SVGF's temporal variance).  Two options, both 0 by default; with
 * both at 0 every call above does exactly what it does without them.  DEFINED bit for bit under the same rules
 * (tests/temporal_moments_mirror.py restates it): binary32, one rounding per operation in the order written, no contraction.
 * Option "temporal_moments": 0 off; 1, 2: rtgl_temporal_accumulate also maintains a MOMENTS record {m1, m2, v, n} per pixel, in two buffers
 * that take turns together with the history buffers (allocated by the first call that needs them, freed with the context); any other value
 * is RTGL_ERR_INVALID.  Per pixel p, with the quantities of the contract above:
 *     x = I.rgb (mode 1)   or   x = I.rgb / d per channel, d = (A > 2^-10) ? A : 2^-10 from the albedo plane, as rtgl_denoise (mode 2)
 *     l = (0.25 x.r + 0.5 x.g) + 0.25 x.b;   ll = l l
 *   in the tap loop, wherever a tap contributes (w > 0; the tap's record Mp(q) is loaded only then):  a1 = a1 + w Mp(q).x;  a2 = a2 + w Mp(q).y
 *   if there is history and ws > 0, al being the colour's blend factor:
 *     h1 = a1 / ws;  h2 = a2 / ws;   m1 = h1 + (l - h1) al;   m2 = h2 + (ll - h2) al
 *   else m1 = l, m2 = ll.
 *     v = m2 - m1 m1;   v = (v > 0) ? v : 0   (a NaN gives 0: v is never a NaN);   the record is {m1, m2, v, n}, n the history length.
 *   The history {out, n} is bit for bit what the call writes with the option off.  Mode 2 needs RTGL_AOV_ALBEDO enabled
 *   (RTGL_ERR_STATE otherwise).  Setting the option to a value different from its current one acts like rtgl_temporal_reset: moments and
 *   colour history always have the same age.  v is the biased sample variance of the frames in the history (times (n - 1) / n of the
 *   unbiased one for a plain mean of n frames).
 *   rtgl_read_temporal_moments_f32 (synchronises; layout of rtgl_read_image_f32) and rtgl_device_temporal_moments (the buffer the LATEST
 *   call wrote: ask again after each call) return RTGL_ERR_STATE / NULL unless the latest successful rtgl_temporal_accumulate stored
 *   moments; a NULL context is RTGL_ERR_INVALID / NULL.
 * Option "denoise_variance": 0 the spatial estimate of rtgl_denoise_guided; 1 the temporal one where the history allows; any other value is
 * RTGL_ERR_INVALID.  rtgl_denoise ignores it.  With 1, rtgl_denoise_guided changes only how v0 is chosen, M being the latest moments record
 * at p and mu, v0s (the v0 of the contract above) and s0 computed exactly as there:
 *     t = (M.w >= 4) and (M.x - M.x == 0) and (M.y - M.y == 0);     v0 = t ? M.z / M.w : v0s
 *   Dividing by the history length makes v0 the variance of the history MEAN, which is what is being filtered; 4 is SVGF's threshold.  Clamp,
 *   passes, vg, the result and the variance buffer {mu, v0, var, s0} follow from that v0, unchanged.  The call then returns
 *   RTGL_ERR_STATE if "denoise_source" is not 1, if the latest rtgl_temporal_accumulate stored no moments, or if the stored mode does not
 *   match the call: mode 2 iff RTGL_DENOISE_DEMODULATE is set, mode 1 iff it is not.
 *   Limit: the firefly clamp does not rescale the v0 of a pixel it scaled down; the over-estimate only widens that pixel's tolerance. */
int rtgl_read_temporal_moments_f32(rtgl_context *ctx, float *rgba);
void *rtgl_device_temporal_moments(rtgl_context *ctx);

/* -- temporal clip: the latest history clamped, in place, into a per-pixel colour box taken from the 7 x 7 geometric neighbourhood of the
 * CURRENT frame, and the history length of a clamped pixel cut (variance clipping, Salvi 2016; the history clamp of ReLAX).
 * rtgl_temporal_accumulate validates the history against geometry only; this call, made after it, is what notices radiance that changed
 * without the first hit changing (a new background, the cube map switched, an edited material, the aperture, a moved light seen in a
 * mirror).  No reference counterpart: the reference resets the image on each of these.  DEFINED bit for bit under the denoisers' rules
 * (tests/temporal_clip_mirror.py restates it): binary32, one rounding per operation in the order written, no contraction, correctly
 * rounded divide and CORRECTLY ROUNDED SQUARE ROOT -- the first contract of this library that takes one (IEEE 754 sqrt, what numpy's
 * float32 sqrt gives).   ew, dot3, in = 1 / (sigma_normal sigma_normal), ip: as in rtgl_denoise.
 *   Inputs, as they are on the context's stream when the call is enqueued: the image I (meant to be this frame's own radiance: the intended
 *   use of rtgl_temporal_accumulate), the planes N and P, the latest history buffer Hc = {rgb, n} (the one rtgl_device_temporal names) and,
 *   if the latest rtgl_temporal_accumulate stored moments, the latest moments buffer.
 *   Geometric weight of a tap q of p:  g(q) = 1;  g = g ew(dot3(N(q).xyz - N(p).xyz) in);  g = g ew(dot3(P(q).xyz - P(p).xyz) ip),
 *     sp = sigma_position P(p).w, ip = (sp > 0) ? 1 / (sp sp) : 0  (a term whose sigma is <= 0 is skipped and its plane is not read; the
 *     position plane is always read for the kind test).
 *   Window, per pixel p: taps j = -3..3 (outer), i = -3..3, q = p + (i, j).  A tap counts only if it is inside the image, is of p's kind,
 *     (P(q).w > 0) == (P(p).w > 0), has g(q) > 0, and c = I(q).rgb is finite in all three channels (c.r - c.r == 0, likewise g and b).
 *     For a tap that counts:  s0 = s0 + g;  per channel  s1 = s1 + g c,  s2 = s2 + g (c c).
 *   Box, if s0 > 0, per channel:  mu = s1 / s0;  v = s2 / s0 - mu mu;  v = (v > 0) ? v : 0;  e = sigma_scale sqrt(v);  lo = mu - e,  hi = mu + e;
 *     then widened so that it always holds the pixel's own sample:  lo = (I(p).c < lo) ? I(p).c : lo;  hi = (I(p).c > hi) ? I(p).c : hi
 *     (without this a noise-free region, a miss on the cube map with DOF off, would be pulled towards its neighbourhood mean).
 *     A pixel ALONE in its window -- no other tap counts: a 1 x 1 image, a hit whose neighbours all fail the geometric tests -- has v = 0 and
 *     the box [I(p), I(p)]: its history is REPLACED by the frame's sample and, if it differed, its length cut.
 *   Clamp, per channel, x = Hc(p).c:  y = (x < lo) ? lo : x;  y = (y > hi) ? hi : y;  the channel is CLIPPED if either compare was true
 *     (a NaN x, lo or hi compares false: it clips nothing and changes nothing).
 *   History length:  n' = (any channel clipped and n > clip_history) ? clip_history : n.     With s0 == 0 nothing changes.
 *   Stores: {y, n'} to Hc(p), in place (a pixel reads and writes only its own record of Hc; the window reads I, N and P only); if moments
 *   are stored, n' to the .w of the pixel's moments record, whose m1, m2 and v stay.  Nothing else is written, no buffer is allocated.
 * Defaults (rtgl_temporal_clip_defaults, and a NULL params): sigma_scale 2, clip_history 3, sigma_normal 0.3, sigma_position 0.05.
 * clip_history 3 puts a clipped pixel under the threshold of 4 of option "denoise_variance": rtgl_denoise_guided then takes its spatial
 * estimate there until the history has grown back.
 * Like its neighbours the call first submits the frames a batching context holds, enqueues one kernel on the context's stream and returns
 * without waiting.  A second call without a new rtgl_temporal_accumulate is allowed and is the identity, bit for bit.  With
 * "denoise_source" = 1 the denoisers filter the clipped history; the next rtgl_temporal_accumulate reprojects it.
 * RTGL_ERR_INVALID: NULL context, a non-finite parameter, sigma_scale <= 0, clip_history < 1, non-zero flags or reserved words.
 * RTGL_ERR_STATE: no rtgl_temporal_accumulate has succeeded; RTGL_AOV_POSITION is not enabled; RTGL_AOV_NORMAL is not enabled while
 * sigma_normal > 0; no frame has been rendered since the planes last restarted; the context is tiled or multi-device.
 * Limits: the box is of raw radiance, not demodulated: texture detail inside a window widens it.  m1, m2 and v of the moments are not
 * clamped: after a change of lighting v over-estimates until the history has regrown.  The box needs I to be ONE frame's radiance: over an
 * accumulating image it narrows as the image converges and ends up clamping the history to the image. */
typedef struct rtgl_temporal_clip_params {
    float    sigma_scale;     /* > 0: half width of the box in standard deviations of the neighbourhood */
    float    clip_history;    /* >= 1: the history length a clipped pixel is cut to */
    float    sigma_normal;    /* <= 0: the normal term of the geometric weight is off (the normal plane is then not needed) */
    float    sigma_position;  /* <= 0: the position term is off; relative to the hit distance, as in rtgl_denoise */
    uint32_t flags;           /* none defined: must be 0 */
    uint32_t reserved[3];     /* must be 0 */
} rtgl_temporal_clip_params;  /* 32 bytes */
int rtgl_temporal_clip_defaults(rtgl_temporal_clip_params *out);
int rtgl_temporal_clip(rtgl_context *ctx, const rtgl_temporal_clip_params *params);

/* -- display transform: one of the float buffers turned into an RGBA8 display buffer ON THE DEVICE: auto exposure from a luminance
 * histogram, a tone curve, and the sRGB transfer function.  rtgl_read_image_u8 stays the reference's glGetTexImage (clamp, x 255, no
 * exposure, no curve, no transfer function, the image only); this is the way out to a picture for scenes whose radiance leaves [0, 1] and
 * for the denoised and the temporal buffers.  No reference counterpart.  DEFINED bit for bit (tests/tonemap_mirror.py restates it), and
 * chosen so that NO TRANSCENDENTAL FUNCTION is needed: integers where the histogram is concerned, binary32 with one rounding per operation
 * in the order written, no contraction and correctly rounded divide elsewhere, two committed tables (raytracer.glsl_amd/csrc/rt_tonemap.hpp;
 * the committed values are the contract):
 *     P[r], r = 0..63   = float32(2^(-r/64))
 *     T[k], k = 1..255  = float32(D((k - 0.5) / 255)) with D the sRGB decoding of IEC 61966-2-1 evaluated in float64,
 *                         D(v) = v / 12.92 for v <= 0.04045, ((v + 0.055) / 1.055)^2.4 above; strictly increasing.
 *   lum(r, g, b) = (0.25 r + 0.5 g) + 0.25 b, as in rtgl_denoise_guided.     S = the source buffer, c = S(p).rgb; S(p).a is not read.
 *   1. Histogram (flag RTGL_TONEMAP_AUTO_EXPOSURE only).  L = lum(c).  A pixel COUNTS iff L > 0: NaN, +0, -0 and negatives go to `ignored`.
 *      Its bin is  b = clamp((bits(L) >> 20) - 888, 0, 255)  in signed integers, bits(L) the 32 bits of L: eight bins per binade, bin 0
 *      beginning at 2^-16 (and holding everything below), bin 255 ending at 2^16 (and holding everything above, +inf included).  h[b] is
 *      the number of counting pixels of bin b: integer sums, independent of any order.
 *   2. Solve (same flag), in 64-bit integers:  N = sum h;  lo = N low_permille / 1000,  hi = N high_permille / 1000  (floor);  walking b
 *      upwards with c the pixels below bin b:  kept[b] = max(0, min(c + h[b], N - hi) - max(c, lo))  -- the darkest lo and the brightest hi
 *      pixels are left out;  K = sum kept[b],  S = sum kept[b] (2 b + 1),  m = 4 S / K (floor),  q = m / 64,  r = m % 64  (m / 64 - 16 is the
 *      mean binary logarithm of the kept luminances, bins taken at their centres).
 *        target = ldexp(key P[r], 16 - q)   (one binary32 multiply, then the exact scaling, rounded once if the result is subnormal);
 *        N == 0:  target = exposure.
 *        e = target;  if adapt < 1 and an exposure `prev` has been stored since the context was created or rtgl_tonemap_reset was called:
 *        e = prev + (target - prev) adapt.     e = (e < exposure_min) ? exposure_min : e;  e = (e > exposure_max) ? exposure_max : e;
 *        e is stored as `prev`.  It never leaves the device inside rtgl_tonemap.
 *      Without the flag steps 1 and 2 are not run: e = exposure as given (not clamped); `prev` and the histogram stay as they were.
 *   3. Map, per channel  x = c e,  then
 *        op RTGL_TONEMAP_LINEAR:    y = x
 *        op RTGL_TONEMAP_REINHARD:  Lx = lum(x);  s = (1 + Lx / (white white)) / (1 + Lx);  y = x s      (luminance mapped, hue kept;
 *                                   a luminance of `white` after exposure maps to 1)
 *        op RTGL_TONEMAP_ACES:      y = (x (2.51 x + 0.03)) / (x (2.43 x + 0.59) + 0.14)                 (Narkowicz's fit, per channel)
 *   4. Encode, per channel:  code = the number of k in 1..255 with T[k] <= y.  This is the correctly rounded sRGB code by comparisons
 *      alone: NaN and negatives give 0, +inf gives 255.  Alpha = 255.  The display buffer is local_rows x width RGBA8 records (bytes r, g,
 *      b, a), rows bottom-up like the image; rtgl_read_display_u8 (synchronises) turns them over if flip != 0, as rtgl_read_image_u8 does.
 * Defaults (rtgl_tonemap_defaults, and a NULL params): source 0, op 1, auto exposure on, exposure 1, key 0.18, white 4, adapt 1,
 * exposure_min 2^-16, exposure_max 2^16, low_permille 100, high_permille 20.
 * Like its neighbours the call first submits the frames a batching context holds, enqueues its kernels on the context's stream (three with
 * auto exposure, one without) and returns without waiting; nothing but the display buffer and the call's own state is written.
 * rtgl_read_tonemap_exposure (synchronises): the e of the latest call.  rtgl_read_tonemap_histogram (synchronises): h and, if `ignored`
 * is not NULL, the ignored pixels, of the latest call WITH auto exposure.  rtgl_device_display: the display buffer (torch interop; valid
 * until the context is destroyed).
 * RTGL_ERR_INVALID: NULL context or output pointer; unknown source, op or flag bits; exposure, key, white, adapt, exposure_min or
 * exposure_max not finite or not > 0; adapt > 1; exposure_min > exposure_max; low_permille + high_permille >= 1000; non-zero reserved.
 * RTGL_ERR_STATE: the source buffer does not exist yet (source 1 before a denoiser call, source 2 before rtgl_temporal_accumulate); the
 * context is tiled or multi-device (the exposure is a property of the whole picture); the read-outs before the first successful call
 * (rtgl_device_display: NULL), rtgl_read_tonemap_histogram before the first one with auto exposure.
 * Limits: no dithering; the histogram weighs every pixel alike, the sky with the subject. */
enum { RTGL_TONEMAP_SOURCE_IMAGE = 0, RTGL_TONEMAP_SOURCE_DENOISED = 1, RTGL_TONEMAP_SOURCE_TEMPORAL = 2 };
enum { RTGL_TONEMAP_LINEAR = 0, RTGL_TONEMAP_REINHARD = 1, RTGL_TONEMAP_ACES = 2 };
enum { RTGL_TONEMAP_AUTO_EXPOSURE = 1 };
typedef struct rtgl_tonemap_params {
    uint32_t source;          /* RTGL_TONEMAP_SOURCE_*: the buffer to display */
    uint32_t op;              /* RTGL_TONEMAP_LINEAR / _REINHARD / _ACES */
    uint32_t flags;           /* bit 0: RTGL_TONEMAP_AUTO_EXPOSURE */
    float    exposure;        /* > 0: used when auto exposure is off, and when no pixel counts */
    float    key;             /* > 0: the value the mean kept luminance is exposed to */
    float    white;           /* > 0: op 1, the luminance after exposure that maps to 1 */
    float    adapt;           /* (0, 1]: the share of the way from the previous exposure to the target taken per call; 1: no memory */
    float    exposure_min;    /* > 0 */
    float    exposure_max;    /* >= exposure_min */
    uint32_t low_permille;    /* the darkest share of the counting pixels left out of the mean, in 1/1000 */
    uint32_t high_permille;   /* the brightest share left out; low_permille + high_permille < 1000 */
    uint32_t reserved[5];     /* must be 0 */
} rtgl_tonemap_params;        /* 64 bytes */
int rtgl_tonemap_defaults(rtgl_tonemap_params *out);
int rtgl_tonemap(rtgl_context *ctx, const rtgl_tonemap_params *params);
int rtgl_tonemap_reset(rtgl_context *ctx);
int rtgl_read_display_u8(rtgl_context *ctx, uint8_t *rgba, int flip);
void *rtgl_device_display(rtgl_context *ctx);
int rtgl_read_tonemap_exposure(rtgl_context *ctx, float *exposure);
int rtgl_read_tonemap_histogram(rtgl_context *ctx, uint32_t hist[256], uint32_t *ignored);

/* -- error estimate: how noisy the accumulation image still is, per 16 x 16 tile and for the whole picture, and the stop rule "render until
 * the picture is this clean" on top of it.  No reference counterpart: the reference renders until somebody saves the image.  The image at
 * two moments of ONE accumulation differs by a known multiple of the noise: with n and m < n real frames in it,
 * Var(mean of n) = E[(mean_n - mean_m)^2] m / (n - m).  One squared difference per pixel is a poor estimate; the mean over a tile or over
 * the picture is a good one.  One streaming pass over the image and a luminance SNAPSHOT of an earlier moment; the frame path is untouched.
 * DEFINED bit for bit under the denoisers' rules (tests/error_mirror.py restates it): binary32, one rounding per operation in the order
 * written, no contraction, correctly rounded divide, integers exact.
 *   lum(r, g, b) = (0.25 r + 0.5 g) + 0.25 b.     W = width, H = height.
 *   Footprint: the pixels with x < W/8*8 and y < H/8*8 (integer division).  The rest of the image is never written by a frame; it is
 *   neither counted nor ignored.     Tiles: 16 x 16 pixels, tx = ceil(W / 16), ty = ceil(H / 16), tile row 0 is buffer row 0.
 *   State: a snapshot plane S of one float per pixel -- the raw lum of the image when it was taken --, the snapshot's F_m and first_frames,
 *   and an epoch kept on the host.  The snapshot is DROPPED by rtgl_error_reset, rtgl_clear_image, rtgl_write_image_f32,
 *   rtgl_bind_device_image, any rendered frame with reset_flag != 0, and by a call whose F_n <= F_m or whose first_frames differs from the
 *   snapshot's.  (That host-side bookkeeping is all this extension adds to those entry points.)
 *   Per call: F_n = the `frames` of the parameters the latest frame was rendered with (frames a batching context holds are submitted
 *   first).  Only rtgl_render_frame counts here: a masked frame (rtgl_adaptive_frame) ignores `frames` and leaves F_n as it was, and a
 *   context that has rendered nothing else has rendered no frame (RTGL_ERR_STATE).  The image after that frame carries the weight F_n + 1 (what the accumulation divides by); first_frames is the `frames` of the
 *   first frame after the image was last zero -- 1 in the reference's loop, 0 for a caller who counts from 0 --, so the image holds
 *   n = F_n + 1 - first_frames real frames and equals their mean times n / (F_n + 1).  n < 1 is RTGL_ERR_INVALID.
 *     g_n = (float)((double)(F_n + 1) / (double)n);   m and g_m likewise from the snapshot's F_m;   c = (float)((double)m / (double)(n - m)).
 *   Per pixel of the footprint, I the image, S the snapshot:
 *     Ln = lum(I.rgb) g_n;  Lm = S g_m;  d = Ln - Lm;  den = ((Ln > 0) ? Ln : 0) + floor;  q = d / den;  e = q q.
 *     The pixel COUNTS iff e - e == 0 (e is finite).  Every other pixel of the footprint goes to `ignored`.
 *   Per tile: sum = the balanced pairwise tree over the 256 row-major indices of the tile (index = 16 row + column): adjacent pairs are
 *     added first, then pairs of pairs, and so on, eight levels; pixels that do not count and positions outside the footprint contribute
 *     +0.  count = the pixels that count (an integer).  mse = (sum / (float)count) c;  converged = count > 0 and mse <= threshold threshold.
 *     A tile with count == 0 has the record {0, 0, 0, 0} and is not VALID.
 *   Whole picture: lane t of 256 adds the tile sums t, t + 256, ... (tile index = tx row + column) in ascending order, starting from +0;
 *     the same 256-leaf tree then combines the lanes to SUM.  N = the sum of the counts;  mse = (SUM / (float)N) c, and 0 if N == 0;
 *     max_tile_mse = the maximum over the valid tiles, 0 if there is none;  tiles_valid, tiles_converged and
 *     pixels_ignored = (footprint pixels) - N are integers;
 *     converged = tiles_valid > 0 and tiles_converged 1000 >= tiles_valid quantile_permille, in 64-bit integers.
 *   No output can be a NaN.  Sums may reach +inf: that is defined and means "not converged".
 *   Snapshot handling: after the estimate the snapshot becomes the current image's lum with F_m = F_n; with RTGL_ERROR_KEEP_SNAPSHOT and
 *   an existing snapshot it is left as it is.  A call without a usable snapshot takes one, writes a summary with valid = 0 and everything
 *   else 0, zeroes the tile records and returns RTGL_OK.
 * Defaults (rtgl_error_defaults, and a NULL params): threshold 0.05, floor 0.01, quantile_permille 950, first_frames 1, flags 0.
 * Like its neighbours the call first submits the frames a batching context holds, enqueues its two kernels on the context's stream and
 * returns without waiting; it writes only its own buffers (snapshot, tile records, summary), which the first call allocates and which are
 * freed with the context: image, planes, RNG states, the denoised, temporal and display buffers are only read or not touched at all.
 * rtgl_read_error_summary and rtgl_read_error_tiles synchronise; the latter copies tx x ty records, row by row, and stores tx and ty
 * where the pointers are not NULL.  rtgl_device_error_tiles: the records on the device (torch interop; valid until the context is destroyed).
 * RTGL_ERR_INVALID: NULL context or output pointer; threshold or floor not finite or not > 0; quantile_permille outside 1..1000;
 * first_frames < 0; unknown flag bits; non-zero reserved words; n < 1; a footprint of 2^32 pixels or more.  RTGL_ERR_STATE: no frame has been rendered on this context; the
 * context is tiled or multi-device (a strip is not the picture; out of scope, like its neighbours); the read-outs before the first
 * successful rtgl_error_estimate (rtgl_device_error_tiles: NULL).
 * Limits: luminance only; radiance not yet seen cannot be estimated from what has been seen, so scenes ridden with fireflies are
 * UNDER-estimated (DESIGN.md 5.10 has figures); a tile that is all sky reads 0 and converged; single-device, untiled contexts only. */
enum { RTGL_ERROR_KEEP_SNAPSHOT = 1 };
typedef struct rtgl_error_params {
    float    threshold;          /* > 0: the relative RMSE a tile must be at or below to be converged */
    float    floor;              /* > 0: added to the luminance a difference is taken relative to */
    uint32_t quantile_permille;  /* 1..1000: the share of the valid tiles that must be converged, in 1/1000 */
    int32_t  first_frames;       /* >= 0: the `frames` of the first frame after the image was last zero */
    uint32_t flags;              /* RTGL_ERROR_KEEP_SNAPSHOT */
    uint32_t reserved[3];        /* must be 0 */
} rtgl_error_params;             /* 32 bytes */
typedef struct rtgl_error_summary {
    uint32_t valid;              /* 1: an estimate; 0: the call only took a snapshot, everything below is 0 */
    uint32_t converged;
    int32_t  frames_now;         /* F_n */
    int32_t  frames_snapshot;    /* F_m */
    uint32_t tiles_valid;
    uint32_t tiles_converged;
    uint32_t pixels_ignored;
    float    scale;              /* c */
    float    mse;                /* relative MSE of the whole picture */
    float    max_tile_mse;
    uint32_t reserved[6];
} rtgl_error_summary;            /* 64 bytes */
typedef struct rtgl_error_tile {
    float    sum;
    float    mse;
    uint32_t count;
    uint32_t converged;
} rtgl_error_tile;               /* 16 bytes */
int rtgl_error_defaults(rtgl_error_params *out);
int rtgl_error_estimate(rtgl_context *ctx, const rtgl_error_params *params);
int rtgl_error_reset(rtgl_context *ctx);                    /* drops the snapshot: the next rtgl_error_estimate takes a new one */
int rtgl_read_error_summary(rtgl_context *ctx, rtgl_error_summary *out);
int rtgl_read_error_tiles(rtgl_context *ctx, rtgl_error_tile *tiles, uint32_t *tx, uint32_t *ty);
void *rtgl_device_error_tiles(rtgl_context *ctx);

/* -- adaptive sampling: frames that trace only the 16 x 16 tiles that are still noisy, with a sample count per tile.  The error estimate
 * above tells a caller how noisy each tile is; this acts on it.  No reference counterpart.  No existing kernel changes: a masked frame is
 * the ordinary per-bounce pipeline behind a ray generator that reads a list of 8 x 8 pixel blocks, traced as a one-frame image into a
 * sample buffer, and a merge kernel folds that buffer into the image with the tile's own count.  DEFINED bit for bit under the rules of
 * rtgl_error_estimate (tests/adaptive_mirror.py restates it): binary32, one rounding per operation in the order written, no contraction,
 * correctly rounded divide, integers exact; lum and the balanced 256-leaf pairwise tree are the ones of rtgl_error_estimate.
 *   Shapes: tiles are 16 x 16, tx = ceil(W / 16), ty = ceil(H / 16), tile index t = tx row + column.  Footprint: the pixels with
 *   x < W/8*8 and y < H/8*8.  Blocks: the 8 x 8 pixel blocks of queue 0, row-major, blocks_x = (W/8*8) / 8; block b lies in the tile
 *   (b / blocks_x / 2, b % blocks_x / 2).
 *   State of a session: a count n[t] per tile, a snapshot plane S (one float per pixel) with its count m[t] per tile, a sample buffer the
 *   size of the image, the tile records; on the host the mask active[t] and the block list: the indices of the footprint blocks that lie
 *   in active tiles, ascending.
 *   rtgl_adaptive_begin validates and stores the parameters, allocates what is missing, zeroes the image exactly as rtgl_clear_image does
 *   (the error snapshot is dropped, the planes' count restarts), zeroes n, m and the records and sets every tile that holds a footprint
 *   pixel active.
 *   rtgl_adaptive_frame renders one frame of one sample over the active tiles.  Camera, random, max_bounce, background, environment and
 *   DOF come from the current rtgl_frame_params; `frames` and `reset_flag` are ignored.  Slot idx of queue 0 is pixel (in & 7, in >> 3) of
 *   block list[idx >> 6], in = idx & 63; n0 = 64 len(list).  Seeds and camera rays use absolute pixel coordinates as always: the sample of
 *   an active pixel is bit for bit the sample the ordinary frame with the same uniforms gives that pixel, whatever the mask.  The frame is
 *   traced as a frame with reset_flag = 1, frames = 0 into the sample buffer, which then holds x = (radiance + 0 0) / 1.  Then per
 *   active tile t and per footprint pixel of it, with k = n[t] and prev the image:
 *     v = (x + prev (float)k) / (float)(k + 1) per channel, alpha 1        (the accumulation's operations with frames = k)
 *   and n[t] = k + 1.  Pixels of inactive tiles and pixels outside the footprint are not written.  With an empty list the call enqueues
 *   nothing and returns RTGL_OK.  Frames a batching context holds are submitted first.  Where the effective kernel would be
 *   RTGL_KERNEL_MEGA (explicit, or a scene without triangles) the frame runs RTGL_KERNEL_WAVEFRONT, and "kernel_in_use" says so.  The frame
 *   neither uses nor leaves kept camera bits and never takes the lean camera bounce.  rtgl_last_frame_ms covers generation through merge.
 *   rtgl_adaptive_update first runs, per tile with n > m:
 *     m == 0: the snapshot is taken (S = lum(I) over the tile's footprint pixels, m = n); the record is {0, 0, 0, 0, n, m}: not valid.
 *     m >= 1: c = (float)m / (float)(n - m);  per footprint pixel  Ln = lum(I);  Lm = S;  d = Ln - Lm;  den = ((Ln > 0) ? Ln : 0) + floor;
 *       q = d / den;  e = q q  (no g factors: both means are unbiased).  The pixel COUNTS iff e - e == 0.  sum = the tree over the tile's 256
 *       row-major indices, pixels that do not count and positions outside the footprint contributing +0;  count = the counting pixels;
 *       mse = (sum / (float)count) c;  converged = count > 0 and mse <= threshold threshold;  count == 0: sum = mse = 0.  Then S = lum(I),
 *       m = n.  The record is {sum, mse, count, converged, n, m}; it is VALID iff count > 0.
 *   A tile with n == m keeps its record and its snapshot.
 *   It then synchronises, reads the records and sets the mask:
 *     active[t] = n < min_samples or (n < max_samples and not (valid and converged));   a tile without footprint pixels is never active.
 *   It rebuilds and uploads the block list and fills the summary (over the tiles that hold a footprint pixel): tiles_total; tiles_active;
 *   tiles_converged = valid and converged records; tiles_capped = n >= max_samples and not (valid and converged); blocks_active = the
 *   list's length; samples_min, samples_max = the smallest and largest n; converged = no tile is active; samples_total = the sum of n over
 *   the footprint's pixels; max_tile_mse = the largest mse of a valid record, 0 without one.
 *   rtgl_adaptive_set_mask replaces the mask by an explicit one, tx x ty bytes, row by row, non-zero = active (a tile without footprint
 *   pixels stays inactive), until the next rtgl_adaptive_update replaces it: this is also region-of-interest rendering.
 *   rtgl_adaptive_get_mask copies the mask as it stands.  rtgl_read_adaptive_tiles (synchronises) copies the tx x ty records and stores tx
 *   and ty where the pointers are not NULL; between updates the records are those of the latest update.  rtgl_device_adaptive_tiles: the
 *   records on the device (valid until the context is destroyed; NULL before the first rtgl_adaptive_begin).
 * Defaults (rtgl_adaptive_defaults): threshold 0.05, floor 0.01, min_samples 16, max_samples 1024, flags 0.
 * RTGL_ERR_INVALID: NULL context, params or output pointer; threshold or floor not finite or not > 0; min_samples < 1; max_samples <
 * min_samples; non-zero flags or reserved words; at rtgl_adaptive_frame: samples != 1 or max_bounce == 0 in the frame parameters.
 * RTGL_ERR_STATE: no session (every call but begin and defaults); rtgl_adaptive_frame without frame parameters or with option "aov" or
 * "rng_state" non-zero; a tiled or multi-device context.
 * rtgl_render_frame, rtgl_clear_image, rtgl_write_image_f32 and rtgl_bind_device_image END the session (their own behaviour is unchanged):
 * the image is no longer the session's.  The next rtgl_adaptive_frame is RTGL_ERR_STATE until a new rtgl_adaptive_begin.
 * rtgl_render_frame ends it when the frame is accepted: a call refused for its parameters (RTGL_ERR_STATE before rtgl_set_frame_params,
 * RTGL_ERR_INVALID for samples == 0, which divides by zero in the reference) leaves the session open.
 * A masked frame drops the snapshot of rtgl_error_estimate, like every other writer of the image that is not a counted frame.
 * Limits: the classic bias of stopping on an estimate (a tile stops when its noise happens to read low); a stopped tile is never
 * re-examined; seams between tiles of different counts; the first-hit planes, RNG states, denoised, temporal and display buffers are not
 * written by masked frames; single-device, untiled contexts only. */
typedef struct rtgl_adaptive_params {
    float    threshold;          /* > 0: the relative RMSE at or below which a tile stops */
    float    floor;              /* > 0: added to the luminance a difference is taken relative to */
    uint32_t min_samples;        /* >= 1: no tile stops below this count */
    uint32_t max_samples;        /* >= min_samples: every tile stops at this count */
    uint32_t flags;              /* none defined: must be 0 */
    uint32_t reserved[3];        /* must be 0 */
} rtgl_adaptive_params;          /* 32 bytes */
typedef struct rtgl_adaptive_tile {
    float    sum;
    float    mse;
    uint32_t count;
    uint32_t converged;
    uint32_t samples;            /* n */
    uint32_t samples_snapshot;   /* m */
    uint32_t reserved[2];
} rtgl_adaptive_tile;            /* 32 bytes */
typedef struct rtgl_adaptive_summary {
    uint32_t tiles_total;        /* tiles that hold a footprint pixel */
    uint32_t tiles_active;
    uint32_t tiles_converged;
    uint32_t tiles_capped;
    uint32_t blocks_active;
    uint32_t samples_min;
    uint32_t samples_max;
    uint32_t converged;          /* 1: no tile is active */
    uint64_t samples_total;
    float    max_tile_mse;
    uint32_t reserved[5];
} rtgl_adaptive_summary;         /* 64 bytes */
int rtgl_adaptive_defaults(rtgl_adaptive_params *out);
int rtgl_adaptive_begin(rtgl_context *ctx, const rtgl_adaptive_params *params);
int rtgl_adaptive_frame(rtgl_context *ctx);
int rtgl_adaptive_update(rtgl_context *ctx, rtgl_adaptive_summary *summary_out);
int rtgl_adaptive_set_mask(rtgl_context *ctx, const uint8_t *tiles);
int rtgl_adaptive_get_mask(rtgl_context *ctx, uint8_t *tiles);
int rtgl_read_adaptive_tiles(rtgl_context *ctx, rtgl_adaptive_tile *tiles, uint32_t *tx, uint32_t *ty);
void *rtgl_device_adaptive_tiles(rtgl_context *ctx);

/* -- robust accumulation: the frames dealt round-robin into K bucket means, and a resolve that drops the buckets that disagree with the
 * others (median of means with a Gini-adaptive trim; Buisine et al., EGSR 2021; Jung et al. 2015).  A firefly stays in a running mean with
 * weight 1/N for the rest of the accumulation; here it stays in one bucket, and the resolve leaves that bucket out where the buckets'
 * luminances are unequal enough.  Where they agree nothing is dropped and the result is the mean.  No reference counterpart.  The frame
 * path, every existing kernel and every existing entry point are untouched: one streaming fold per frame, one resolve when the picture
 * is wanted.  DEFINED bit for bit under the rules of rtgl_error_estimate (tests/robust_mirror.py restates it): binary32, one rounding per
 * operation in the order written, no contraction, correctly rounded divide, subnormals kept, integers exact; (float) of an integer is
 * exact here.  Where a result is a NaN is defined; the NaN's sign and payload are not.
 *   State of a session: K planes of the context's rows (local_rows x width float4, bucket-major), one output plane of that size, the
 *   frame count N.  All of it is allocated by rtgl_robust_begin and freed by rtgl_robust_end: a context that never begins holds none.
 *   rtgl_robust_begin validates the parameters, allocates (a second begin restarts the session and reallocates only if K changed),
 *   zeroes the planes and sets N = 0.
 *   rtgl_robust_accumulate folds the accumulation image AS IT STANDS, taken as one sample x, into bucket j = N mod K, which holds
 *   k = N div K samples, per component, x, y, z and w alike:
 *     b' = (x + b (float)k) / (float)(k + 1)                             (the accumulation's operations with frames = k)
 *   then N = N + 1.  The caller renders each frame with reset_flag = 1, frames = 0, so that the image holds one frame's radiance; the call
 *   cannot check that, and folds whatever the image holds.  Frames a batching context holds are submitted first.  The image, the counters
 *   of rtgl_error_estimate and an adaptive session are not touched.
 *   rtgl_robust_resolve needs N >= 1.  With n_j = N div K + (j < N mod K ? 1 : 0), per pixel:
 *     1. l_j = (0.25 r + 0.5 g) + 0.25 b of bucket j                     (lum of rtgl_error_estimate)
 *     2. key_j = l_j if l_j is finite, else +inf
 *     3. rank_j = the number of i != j with key_i < key_j or (key_i == key_j and i < j)
 *     4. S = the keys added to +0 one by one in bucket order
 *     5. A = the products (float)(2 rank_j - (K - 1)) key_j added to +0 one by one in bucket order
 *     6. G = 1 if S is not finite; else G = 0 if not S > 0; else G = A / ((float)K S).  Then G = 1 if not G <= 1; then G = 0 if not G >= 0.
 *     7. u = (G gain) (float)(K / 2);  t = (K - 1) / 2 if u >= (float)((K - 1) / 2), else (int)u (truncated);  t = 0 while N < K.
 *     8. bucket j is KEPT iff n_j > 0 and t <= rank_j <= K - 1 - t.
 *     9. W = the (float)n_j of the kept buckets added to +0 one by one in BUCKET order; C = the products (float)n_j b_j likewise, per
 *        component, w included;  out = C / W.
 *   G is the Gini coefficient of the bucket luminances; K / 2 G buckets go at either end, at least one (K even: two) stays.
 *   dest = RTGL_ROBUST_DEST_BUFFER stores {out.x, out.y, out.z, G} in the output plane, which rtgl_read_robust_f32 reads; nothing else
 *   changes.  dest = RTGL_ROBUST_DEST_IMAGE stores out, all four components, in the accumulation image and does on the host what
 *   rtgl_write_image_f32 does: an adaptive session ends, the snapshot of rtgl_error_estimate is dropped, the first-hit planes and their
 *   count stay as they are.  rtgl_denoise*, rtgl_tonemap and save_to_file then take the picture like any image.  The session goes on
 *   after either.  gain = 0 is the plain weighted mean of the buckets.
 *   rtgl_robust_end frees the planes.  rtgl_robust_frames stores N and K where the pointers are not NULL.  rtgl_read_robust_f32 copies
 *   the output plane of the latest resolve with dest BUFFER, rtgl_read_robust_bucket_f32 the plane of one bucket (both synchronise; the
 *   context's rows, as rtgl_read_image_f32 of a single-device context gives them).
 * A tiled context (rtgl_create_tiled) works on its own strips: there is no neighbourhood.
 * Defaults (rtgl_robust_defaults; either pointer may be NULL, not both): buckets 8, flags 0; gain 1, dest 0, flags 0.
 * RTGL_ERR_INVALID: NULL context, params or output pointer (rtgl_robust_frames: both NULL); buckets not 4, 8 or 16; gain NaN, negative or
 * infinite; dest > 1; non-zero flags or reserved words; bucket >= K.
 * RTGL_ERR_STATE: no session (every call but begin and defaults: before the first begin and after rtgl_robust_end); rtgl_robust_resolve
 * with N = 0; rtgl_read_robust_f32 before a resolve with dest BUFFER; rtgl_robust_accumulate after 2^32 - 1 frames; a multi-device context
 * (rtgl_create_multi).
 * Limits: a trimmed estimator loses energy where it trims (3-5 % on the measured firefly scenes); it is biased for N finite and
 * consistent as N grows; the ranks are of luminance, so an outlier in hue at equal luminance passes; K = 16 with under about 4 samples
 * per bucket trims smooth pixels too; memory is 16 (K + 1) bytes per pixel. */
typedef struct rtgl_robust_params {
    uint32_t buckets;            /* K: 4, 8 or 16 */
    uint32_t flags;              /* none defined: must be 0 */
    uint32_t reserved[6];        /* must be 0 */
} rtgl_robust_params;            /* 32 bytes */
typedef struct rtgl_robust_resolve_params {
    float    gain;               /* finite, >= 0: scales the trim; 0: the weighted mean */
    uint32_t dest;               /* RTGL_ROBUST_DEST_* */
    uint32_t flags;              /* none defined: must be 0 */
    uint32_t reserved[5];        /* must be 0 */
} rtgl_robust_resolve_params;    /* 32 bytes */
enum { RTGL_ROBUST_DEST_BUFFER = 0, RTGL_ROBUST_DEST_IMAGE = 1 };
int rtgl_robust_defaults(rtgl_robust_params *params, rtgl_robust_resolve_params *resolve_params);
int rtgl_robust_begin(rtgl_context *ctx, const rtgl_robust_params *params);
int rtgl_robust_accumulate(rtgl_context *ctx);
int rtgl_robust_resolve(rtgl_context *ctx, const rtgl_robust_resolve_params *params);
int rtgl_robust_end(rtgl_context *ctx);
int rtgl_robust_frames(rtgl_context *ctx, uint32_t *frames, uint32_t *buckets);
int rtgl_read_robust_f32(rtgl_context *ctx, float *rgba);
int rtgl_read_robust_bucket_f32(rtgl_context *ctx, uint32_t bucket, float *rgba);

/* -- robust error estimate: the noise level of the picture rtgl_robust_resolve makes, and the stop rule of a robust session.  The K
 * buckets of an open session are K independent estimates of every pixel; their spread, taken over the buckets the resolve keeps, is an
 * estimate of the noise of the picture the resolve makes (Yuen's standard error of a trimmed mean: the variance of the WINSORIZED
 * luminances over h (h - 1), h the buckets kept).  rtgl_error_estimate needs an accumulating image and cannot serve a session, whose
 * image is reset every frame.  No reference counterpart.  Every existing kernel and entry point is untouched.  DEFINED bit for bit under
 * the rules of rtgl_error_estimate (tests/robust_error_mirror.py restates it): binary32, one rounding per operation in the order written,
 * no contraction, correctly rounded divide, subnormals kept, integers exact.  rtgl_error_summary and rtgl_error_tile are reused as they
 * are; footprint, tiles, lum and the balanced 256-leaf pairwise tree are those of rtgl_error_estimate.
 *   Per footprint pixel, with K, N and the bucket planes of the open session:
 *     1. steps 1-7 of rtgl_robust_resolve with THIS call's gain: key_j, rank_j, S, A, G, t
 *     2. lo = the key of the bucket with rank t;  hi = the key of the bucket with rank K - 1 - t
 *     3. w_j = min(max(key_j, lo), hi)                                   (the winsorized keys)
 *     4. M = the w_j added to +0 one by one in bucket order;  mw = M / (float)K
 *     5. D = the squares (w_j - mw) (w_j - mw) added to +0 one by one in bucket order
 *     6. T = the key_j of the kept buckets (t <= rank_j <= K - 1 - t) added to +0 one by one in bucket order
 *     7. h = K - 2 t;  mu = T / (float)h;  v = D / (float)(h (h - 1))    (with t = 0 the textbook s^2 / K)
 *     8. den = ((mu > 0) ? mu : 0) + floor;  e = v / (den den)
 *     9. the pixel COUNTS iff e - e == 0
 *   h >= 2 always: K is even and t is at most (K - 1) / 2.  The buckets are taken as EQUALLY weighted: their sample counts differ by at
 *   most one (n_j of rtgl_robust_resolve), and mu is the plain mean of the kept keys, not the resolve's weighted one.
 *   Per tile: sum = the e of the pixels that count by the tree (the others and positions outside the footprint: +0), count,
 *   mse = sum / (float)count (there is no scale: c = 1), converged = count > 0 and mse <= threshold threshold; a tile with count == 0
 *   has the record {0, 0, 0, 0}.
 *   Whole picture: the solve of rtgl_error_estimate with c = 1 and valid = 1.  The summary carries frames_now = (int32_t)N,
 *   frames_snapshot = 0 and scale = 1.
 *   State: the tile records and the summary are buffers of the SESSION, allocated by its first estimate and freed by rtgl_robust_end; a
 *   second rtgl_robust_begin keeps the memory, and the read-outs wait for the new session's first estimate.  The call writes nothing else:
 *   the buckets, the output plane, the image, the first-hit planes, the snapshot and the records of rtgl_error_estimate and an adaptive
 *   session are only read or not touched.  It submits held frames first, enqueues on the context's stream and returns without waiting;
 *   rtgl_read_robust_error_summary and rtgl_read_robust_error_tiles synchronise (the latter copies tx x ty records and stores tx and ty
 *   where the pointers are not NULL).  rtgl_device_robust_error_tiles: the records on the device, valid until rtgl_robust_end.
 * Defaults (rtgl_robust_error_defaults; rtgl_robust_error_estimate with params NULL): threshold 0.05, floor 0.01, gain 1, quantile 950, flags 0.
 * RTGL_ERR_INVALID: NULL context or output pointer; threshold or floor not finite or not > 0; gain NaN, negative or infinite;
 * quantile_permille outside 1..1000; non-zero flags or reserved words.
 * RTGL_ERR_STATE: no session; N < K (an empty bucket has no luminance); a tiled or multi-device context (a strip is not the picture); the
 * read-outs before the first successful estimate of the session (rtgl_device_robust_error_tiles: NULL).
 * Limits: luminance only; on firefly scenes the estimate reads LOW at small N (a firefly not yet drawn is in no bucket); K = 16 is
 * unreliable below about 16 samples per bucket; the bias of the trim itself is not seen; equal bucket weights are assumed. */
typedef struct rtgl_robust_error_params {
    float    threshold;          /* > 0, finite: relative RMSE a tile must be at or below */
    float    floor;              /* > 0, finite */
    float    gain;               /* finite, >= 0: the resolve's gain; the estimate is of THAT picture */
    uint32_t quantile_permille;  /* 1..1000 */
    uint32_t flags;              /* none defined: must be 0 */
    uint32_t reserved[3];        /* must be 0 */
} rtgl_robust_error_params;      /* 32 bytes */
int rtgl_robust_error_defaults(rtgl_robust_error_params *out);
int rtgl_robust_error_estimate(rtgl_context *ctx, const rtgl_robust_error_params *params);
int rtgl_read_robust_error_summary(rtgl_context *ctx, rtgl_error_summary *out);
int rtgl_read_robust_error_tiles(rtgl_context *ctx, rtgl_error_tile *tiles, uint32_t *tx, uint32_t *ty);
void *rtgl_device_robust_error_tiles(rtgl_context *ctx);

/* -- robust denoise: the resolve of an open robust session and the filter of rtgl_denoise_guided in one call, the luminance tolerance of
 * every pixel taken from the spread of its own K bucket means.  rtgl_denoise_guided sees one picture and estimates a pixel's variance
 * from a 7 x 7 window of that picture's luminance: fine texture counts as noise there and is blurred, and a noisy but locally flat region
 * gets too tight a tolerance.  The K buckets are K independent estimates of the pixel itself; Yuen's variance of the trimmed mean (robust
 * error estimate, step 7) is the variance of the very picture being filtered, per pixel.  No reference counterpart.  Every existing kernel,
 * option and entry point is untouched.  DEFINED bit for bit under the rules of its neighbours (tests/robust_denoise_mirror.py restates
 * it): binary32, one rounding per operation in the order written, no contraction, correctly rounded divide, subnormals kept, integers
 * exact.
 *   Per pixel, with K, N and the bucket planes b_j of the open session, A, N and P the first-hit planes as they are on the stream:
 *     1. steps 1-9 of rtgl_robust_resolve with THIS call's gain: l_j, key_j, rank_j, t, the kept buckets and out, all four components
 *     2. d = the divisor of rtgl_denoise, per channel (A > 2^-10) ? A : 2^-10;  c0 = out.rgb / d when RTGL_DENOISE_DEMODULATE is set,
 *        else c0 = out.rgb
 *     3. x_j = lum(b_j.r / d.r, b_j.g / d.g, b_j.b / d.b) when demodulating, else x_j = l_j;  then x_j = +inf if it is not finite
 *        (lum of rtgl_denoise_guided)
 *     4. lo = the x of the bucket with rank t;  hi = the x of the bucket with rank K - 1 - t;
 *        w_j = lo if rank_j < t;  hi if rank_j > K - 1 - t;  else x_j      (winsorized by the RESOLVE's ranks: with a per-channel albedo
 *        the order of the x can differ from the order of the keys, and the trim must be the resolve's)
 *     5. M, mw and D as in steps 4-5 of the robust error estimate, over these w_j;  h = K - 2 t;  v = D / (float)(h (h - 1));
 *        v0 = v if v - v == 0, else +0.   Without demodulation v is, bit for bit, the v of rtgl_robust_error_estimate step 7 for the
 *        same gain.
 *     6. the NEAR neighbours of rtgl_denoise_guided: those of the 3 x 3 about p inside the image with geometric weight g > 0, the same g
 *     7. the passes of rtgl_denoise_guided, unchanged, over the records {c0, v0} in place of {c1, v0}: "Pass L = 0 .. passes-1" there.
 *        Result: rgb = demodulating ? c d : c,  a = out.w.  The VARIANCE buffer holds {lum(c0), v0, var after the last pass, (float)h}.
 *   There is no firefly clamp and no spatial estimate: the trim is the session's treatment of fireflies.  passes = 0 without
 *   demodulation gives the DENOISED buffer equal to the resolve's out, bit for bit.
 *   The result is in the DENOISED and the VARIANCE buffer of the denoisers: rtgl_read_denoised_f32, rtgl_device_denoised,
 *   rtgl_read_denoise_variance_f32, rtgl_device_denoise_variance and source 1 of rtgl_tonemap take it as they take rtgl_denoise_guided's.
 *   The call submits held frames first, enqueues on the context's stream and returns without waiting.  It writes the denoised buffer, the
 *   two scratch buffers, the variance buffer and the near buffer (allocated by the first call that needs them, freed with the context) and
 *   nothing else: the buckets, the output plane and the session's error records are only read or not touched, and so are the image, the
 *   first-hit planes, the snapshot of rtgl_error_estimate and an adaptive session.  The session goes on.
 * Defaults (rtgl_robust_denoise_defaults, and a NULL params): passes 5, sigma_lum 4, sigma_normal 0.3, sigma_position 0.05, gain 1,
 * demodulate on.
 * RTGL_ERR_INVALID: NULL context, passes > 8, a non-finite sigma, sigma_lum <= 0, gain NaN, negative or infinite, unknown flag bits,
 * non-zero reserved words.
 * RTGL_ERR_STATE: no session; N < K (an empty bucket has no luminance); a tiled or multi-device context; a plane the parameters need is
 * not enabled; a plane is needed and no frame has been rendered since the planes last restarted (the conditions of rtgl_denoise_guided).
 * Limits: a session renders every frame with reset_flag = 1, so the first-hit planes hold the LATEST frame's jittered hit, not a mean
 * over the session: edges of the guides are one sample's.  Accumulating the guides over a session is out of scope.  The variance is of
 * the luminance only; K = 4 gives 3 degrees of freedom or fewer per pixel, and the passes' own 3 x 3 blur of the variance is what
 * steadies it. */
typedef struct rtgl_robust_denoise_params {
    uint32_t passes;          /* 0..8 */
    float    sigma_lum;       /* > 0: luminance tolerance in standard deviations */
    float    sigma_normal;    /* <= 0: the normal term is off */
    float    sigma_position;  /* <= 0: the position term is off; relative to the hit distance */
    float    gain;            /* finite, >= 0: the resolve's gain */
    uint32_t flags;           /* RTGL_DENOISE_DEMODULATE */
    uint32_t reserved[2];     /* must be 0 */
} rtgl_robust_denoise_params; /* 32 bytes */
int rtgl_robust_denoise_defaults(rtgl_robust_denoise_params *out);
int rtgl_robust_denoise(rtgl_context *ctx, const rtgl_robust_denoise_params *params);

/* -- robust adaptive sampling: a session whose sample count is per 16 x 16 tile AND whose samples go into K bucket means.  Adaptive
 * sampling spends frames only where the picture is noisy but keeps every firefly in a running mean and stops on two moments of that mean;
 * a robust session removes the fireflies and estimates the noise of the picture it makes, but traces the whole picture every frame.  This
 * is the third kind of session, next to those two: masked frames (the ordinary per-bounce pipeline behind a block list, as in adaptive
 * sampling) folded into the bucket of each tile's own next sample, the spread estimate per tile whose count has moved, the mask rule of
 * adaptive sampling, and a resolve that takes every pixel's N from its tile.  No reference counterpart.  No existing kernel, option or
 * entry point changes; rtgl_adaptive_tile, rtgl_adaptive_summary and rtgl_robust_resolve_params are reused as they are.  DEFINED bit for
 * bit under the rules of its neighbours (tests/robust_adaptive_mirror.py restates it): binary32, one rounding per operation in the order
 * written, no contraction, correctly rounded divide, subnormals kept, integers exact; (float) of every count is exact (max_samples <=
 * 2^24).  Where a result is a NaN is defined; the NaN's sign and payload are not.
 *   Shapes, footprint, tiles and blocks are those of adaptive sampling.  Single-device, untiled contexts only.
 *   State of a session, all of it the session's own, allocated by rtgl_robust_adaptive_begin and freed by rtgl_robust_adaptive_end: K
 *   bucket planes of the image's size (float4, bucket-major), a count n[t] and an estimate count m[t] per tile, the tile records, a sample
 *   buffer and an output plane of the image's size; on the host the mask active[t], the block list and the tile list.  The session is
 *   independent of an adaptive session and of a robust session: either may be open beside it, and neither is read or written.  The events
 *   that end an adaptive session do not end this one: only rtgl_robust_adaptive_end does.
 *   rtgl_robust_adaptive_begin validates the parameters, allocates what is missing (a second begin restarts the session and reallocates
 *   only if K changed), zeroes the buckets, n, m and the records and sets active every tile that holds a footprint pixel.  It does not
 *   touch the image.
 *   rtgl_robust_adaptive_frame renders one frame of one sample over the active tiles, exactly as rtgl_adaptive_frame does (the same
 *   uniforms taken and ignored, the same block indirection, the same sample for an active pixel whatever the mask, RTGL_KERNEL_WAVEFRONT
 *   where the effective kernel would be RTGL_KERNEL_MEGA, no kept camera bits used or left), traced with reset_flag = 1, frames = 0 into
 *   the session's sample buffer, and then runs the FOLD with that buffer as the source.  It writes neither the image nor anything of
 *   rtgl_error_estimate.  With an empty list the call enqueues nothing and returns RTGL_OK.  Frames a batching context holds are submitted
 *   first.  rtgl_last_frame_ms covers generation through the fold.
 *   The FOLD: per active tile t and per footprint pixel of it, with n = n[t], j = n mod K, k = n div K, x the source pixel and b the pixel
 *   of bucket j:
 *     b' = (x + b (float)k) / (float)(k + 1) per component, w included        (rtgl_robust_accumulate's operations)
 *   then n[t] = n + 1.  Pixels of inactive tiles and pixels outside the footprint are not written.
 *   rtgl_robust_adaptive_accumulate submits held frames, then runs the fold with the accumulation image AS IT STANDS as the source: for
 *   frames the caller rendered some other way.
 *   rtgl_robust_adaptive_update first runs, per tile with n != m:
 *     n < K:  the record is {0, 0, 0, 0, n, n}: not valid.
 *     n >= K: steps 1-9 of rtgl_robust_error_estimate per footprint pixel, with the session's gain and floor (t is never zeroed: every
 *       bucket holds a sample; the buckets are taken as equally weighted);  sum = the e of the pixels that count by the 256-leaf tree over
 *       the tile's row-major indices, the others and positions outside the footprint contributing +0;  count = the counting pixels;
 *       mse = sum / (float)count;  converged = count > 0 and mse <= threshold threshold;  count == 0: {0, 0, 0, 0}.  The record is
 *       {sum, mse, count, converged, n, n}; it is VALID iff count > 0.
 *     In both cases m = n afterwards.
 *   A tile with n == m keeps its record and is not read: a stopped tile costs nothing per update.
 *   It then synchronises, reads the records, sets the mask by the rule of rtgl_adaptive_update with min_samples and max_samples, rebuilds
 *   and uploads the lists and fills the summary as rtgl_adaptive_update does.
 *   rtgl_robust_adaptive_set_mask, rtgl_robust_adaptive_get_mask and rtgl_read_robust_adaptive_tiles behave as their rtgl_adaptive_*
 *   namesakes, on this session.  rtgl_device_robust_adaptive_tiles: the records on the device, valid until rtgl_robust_adaptive_end; NULL
 *   without a session.
 *   rtgl_robust_adaptive_resolve, per pixel of the image, with N = n[t] of the pixel's tile:
 *     a pixel outside the footprint, or with N == 0, gets {+0, +0, +0, +0} (G = +0);
 *     otherwise steps 1-9 of rtgl_robust_resolve with that N: n_j = N div K + (j < N mod K ? 1 : 0), t = 0 while N < K, empty buckets
 *     not kept.
 *   dest = RTGL_ROBUST_DEST_BUFFER stores {out.x, out.y, out.z, G} in the session's output plane, which rtgl_read_robust_adaptive_f32
 *   reads; nothing else changes.  dest = RTGL_ROBUST_DEST_IMAGE stores all four components in the accumulation image and does on the host
 *   exactly what rtgl_robust_resolve with dest IMAGE does: an adaptive session ends, the snapshot of rtgl_error_estimate is dropped.  The
 *   session goes on after either.
 *   rtgl_read_robust_adaptive_bucket_f32 copies the plane of one bucket (synchronises).
 * Defaults (rtgl_robust_adaptive_defaults): buckets 8, threshold 0.05, floor 0.01, gain 1, min_samples 32, max_samples 1024, flags 0.
 * RTGL_ERR_INVALID: NULL context, params or output pointer; buckets not 4, 8 or 16; threshold or floor not finite or not > 0; gain NaN,
 * negative or infinite; min_samples < K; max_samples < min_samples or > 16777216; non-zero flags or reserved; bucket >= K; dest > 1; at
 * rtgl_robust_adaptive_frame: samples != 1 or max_bounce == 0 in the frame parameters.
 * RTGL_ERR_STATE: no session (every call but begin and defaults); a tiled or multi-device context; rtgl_read_robust_adaptive_f32 before a
 * resolve with dest BUFFER; rtgl_robust_adaptive_frame without frame parameters or with option "aov" or "rng_state" non-zero.
 * Every refusal sets a text in rtgl_last_error that names the call.
 * Limits: those of both parents -- the trim loses energy where it trims; the estimate reads low while a firefly has not been drawn, so
 * min_samples matters; a stopped tile is never re-examined; seams between tiles of different counts; rtgl_robust_denoise and
 * rtgl_robust_error_estimate serve the plain robust session only; memory is 16 (K + 2) bytes per pixel. */
typedef struct rtgl_robust_adaptive_params {
    uint32_t buckets;            /* K: 4, 8 or 16 */
    float    threshold;          /* > 0, finite: relative RMSE at or below which a tile stops */
    float    floor;              /* > 0, finite */
    float    gain;               /* finite, >= 0: the resolve's gain; the estimate is of THAT picture */
    uint32_t min_samples;        /* >= K */
    uint32_t max_samples;        /* min_samples .. 16777216, so that (float) of every count is exact */
    uint32_t flags;              /* none defined: must be 0 */
    uint32_t reserved;           /* must be 0 */
} rtgl_robust_adaptive_params;   /* 32 bytes */
int rtgl_robust_adaptive_defaults(rtgl_robust_adaptive_params *out);
int rtgl_robust_adaptive_begin(rtgl_context *ctx, const rtgl_robust_adaptive_params *params);
int rtgl_robust_adaptive_frame(rtgl_context *ctx);
int rtgl_robust_adaptive_accumulate(rtgl_context *ctx);
int rtgl_robust_adaptive_update(rtgl_context *ctx, rtgl_adaptive_summary *summary_out);
int rtgl_robust_adaptive_set_mask(rtgl_context *ctx, const uint8_t *tiles);
int rtgl_robust_adaptive_get_mask(rtgl_context *ctx, uint8_t *tiles);
int rtgl_robust_adaptive_resolve(rtgl_context *ctx, const rtgl_robust_resolve_params *params);
int rtgl_robust_adaptive_end(rtgl_context *ctx);
int rtgl_read_robust_adaptive_f32(rtgl_context *ctx, float *rgba);
int rtgl_read_robust_adaptive_bucket_f32(rtgl_context *ctx, uint32_t bucket, float *rgba);
int rtgl_read_robust_adaptive_tiles(rtgl_context *ctx, rtgl_adaptive_tile *tiles, uint32_t *tx, uint32_t *ty);
void *rtgl_device_robust_adaptive_tiles(rtgl_context *ctx);
/* keys: "kernel" (enum above), "wf_rays" (rays per lane 1/2/4/8), "wf_mode" (0 scalar-fed, 1 LDS tiles),
 * "wf_chunk" (triangles per work item of the split intersect kernel, a multiple of 64 in [64, 4096]), "wf_early" (leading bounces
 * that use the wave-level edge short circuit), "wf_packed" (v_pk_fma_f32 ray pairs on/off), "mf_chunk_quads" (kernel 4: 40-triangle quads
 * per work item = per block's LDS-resident chunk, 1..32), "scan_waves" (waves per SIMD of the kernel-4 scan: 0 default (= 2), 1, 2), "scan_dynamic" (work distribution of the kernel-4 scan: 0 chosen by the mesh (default), 1 static turns, 2 dynamic claims, 3 planned equal-cost intervals, 4 turns + a claimed tail),
 * "narrow_fused" (kernel 4, also RTGL_AMD_NARROW_FUSED, read when a context is created: who gives the survivors of the scan their exact test.  0: narrow_phase_kernel,
 * launched behind every scan launch; 1 (default): every scan wave tests the records of its own candidate region when it has run out of work items, beside the waves that are still
 * scanning, and narrow_phase_kernel is not launched.  The image is the same bit for bit -- hits merge by an atomic minimum -- on every path: single frames, "frame_batch", the
 * strips of a rank), "camera_lean" (kernel 4, also RTGL_AMD_CAMERA_LEAN, read when a context is created: the camera-ray bounce of a frame that is culled from the keep
 * bits an earlier frame left -- same camera, image and scene, a single frame of one sample, "aov" off.  1 (default): ray generation stores only what the scan reads (origin,
 * direction, hit key) and the shade launch of that bounce rebuilds each camera ray from its queue slot instead of loading it; 0: every
 * camera ray travels through the queue in full.  Every other frame runs as with 0.  The image is the same bit for bit), "shade_pass" (the wavefront kernels, also
 * RTGL_AMD_SHADE_PASS, read when a context is created: the form of a bounce's shade launch.  1 (default): one pass, a block per 256 slots of the camera queue -- the
 * one bound on a queue's length that the host knows exactly -- unless fewer than one block in 64 is expected to find rays; 0: every launch in grid-stride passes with a
 * grid from the previous frames' ray counts, as before.  The image is the same bit for bit), "cull" (packet culling: a granule of 128 rays skips the tiles
 * of 10 triangles for which every one of its rays is certified to be rejected by the reference's own test: 0 off, 1 on the camera-ray
 * bounce, 2 on every bounce with the queues as they come, 3 (default) on the camera-ray bounce and on every bounce whose queue was BINNED
 * -- moved into (direction cell, origin cell) order between the bounces, which is what makes its granules coherent), "sort_min_rays"
 * (cull 3: a bounce's queue is binned when at least this many rays are expected, default 131072), "mf_group_quads" (quads
 * sharing one local origin: a power of two up to 64; changing it rebuilds the broad-phase data at the next frame),
 * "rng_state", "counters", "aov" (first-hit planes, above), "denoise_source" (what the denoisers filter, above: 0 the image, 1 the temporal history), "temporal_moments" and "denoise_variance" (temporal luminance moments, above), "kernel_timing" (0 off; N > 0: every N-th frame since the last rtgl_timing_reset carries HIP
 * event pairs around its dominant-kernel launches), "frame_batch" (1 (default) .. 16, also RTGL_AMD_FRAME_BATCH: with B > 1 rtgl_render_frame
 * only records the frame until B frames are waiting, then traces them in ONE set of launches and applies their results to the image in
 * frame order -- bit-identical to frame-by-frame, B times the rays per launch (what a rank of a multi-GPU run lacks).  Every other entry
 * point submits the waiting frames first, so the image a caller reads is always complete; frames that differ in samples, bounce limit,
 * environment switch or background close a batch early; with "counters", "rng_state", "aov" or "kernel_timing" on, with more than one sample
 * per frame and for scenes without triangles frames are rendered one by one; rtgl_destroy submits frames that are still waiting;
 * rtgl_device_image returns NULL when that submission fails), "debug_skip_exact" (set only -- rtgl_get_option does not know it.  Timing
 * diagnostics of kernel 4: 0 (default) off; 1 the scan's survivors are dropped instead of tested and 2 the broad phase rejects everything:
 * the image is WRONG for both; 3 every segment goes through the list loop, image unchanged) */
int rtgl_set_option(rtgl_context *ctx, const char *key, int value);
/* rtgl_get_option answers every key above but "debug_skip_exact" with the option's value, except "mf_group_quads": that is the value in use
 * (the option takes effect when the next frame rebuilds the broad-phase data).  It also answers read-only keys: "kernel_in_use" (the
 * variant the last frame ran, -1 before the first); "mf_sets" (kernel 4: the 32-ray sets per scan wave, a constant of the build);
 * "camera_lean_frames" (the frames of this context that took the lean camera bounce, option "camera_lean": tells a taken path from a
 * fallback); "shade_pass_launches" (the shade launches of this context that made one pass, option "shade_pass"); "cand_region_pairs"
 * (kernel 4: the current capacity, in records, of one scan wave's region of the candidate buffer); "device_mbytes" (the device memory this
 * context holds, MiB rounded up) */
int rtgl_get_option(rtgl_context *ctx, const char *key, int *value);
/* elapsed GPU milliseconds of the last rtgl_render_frame (HIP events on the context's stream) */
int rtgl_last_frame_ms(rtgl_context *ctx, float *ms);
/* Per-kernel GPU time of the last frame, from HIP events recorded around every launch of the dominant
 * kernel on the context's stream.  Needs option "kernel_timing"=1 before rendering. */
typedef struct rtgl_frame_timing {
    float    frame_ms;            /* whole frame, first launch to last */
    float    intersect_ms;        /* sum over the ray x triangle kernel launches (the path-trace megakernel when kernel = 0) */
    uint32_t intersect_launches;
    uint32_t reserved;
} rtgl_frame_timing;
int rtgl_last_frame_timing(rtgl_context *ctx, rtgl_frame_timing *out);
/* Same figures summed over every frame rendered since the last rtgl_timing_reset (or since "kernel_timing"
 * was enabled): lets a caller keep frames queued back to back and read the HIP-event times once at the
 * end.  frames_out (may be NULL) receives the number of frames covered.  Synchronises. */
int rtgl_accumulated_timing(rtgl_context *ctx, rtgl_frame_timing *out, uint32_t *frames_out);
int rtgl_timing_reset(rtgl_context *ctx);

#ifdef __cplusplus
}
#endif
#endif /* RTGL_AMD_H */

// The host half of rtgl_guides_frame (include/rtgl_amd.h, "guide pass"), as plain host C++: no HIP in this header, so that the host compiler
// can build it alone (tests/cpp/guides_plan_check.cpp).  What the call refuses and in which order, how the planes' frame count moves, which
// intersect stage finds the mesh hit of the camera rays for which (option "kernel", triangle visits), the launches of the pass and what
// of a context the pass writes.  tests/guides_mirror.py restates the count and the fold.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rt_guides_plan {

constexpr int kOk = 0, kErrInvalid = -1, kErrState = -4;      // (RTGL_OK, RTGL_ERR_INVALID, RTGL_ERR_STATE)
constexpr int kKernelSplit = 2, kKernelSolo = 4;              // (RTGL_KERNEL_WAVEFRONT_SPLIT, RTGL_KERNEL_WAVEFRONT_MFMA_SOLO)

// ---- refusals: the first that applies, in this order.  A refused call moves neither the planes nor their count.
struct Refusal { int code; const char *why; };                // why == NULL: the call goes ahead
inline Refusal refused(bool have_context, bool multi_device, bool have_params, uint32_t aov)
{
    if (!have_context) return {kErrInvalid, "the context is NULL"};
    if (multi_device) return {kErrState, "rtgl_guides_frame: a multi-device handle renders no guide pass; make the call on single-device or tiled contexts"};
    if (!have_params) return {kErrState, "rtgl_guides_frame: rtgl_set_frame_params has not been called"};
    if (aov == 0u) return {kErrState, "rtgl_guides_frame: no first-hit plane is enabled (option \"aov\" is 0)"};
    return {kOk, nullptr};
}

// ---- the planes' count: the pass is one more entry of their running mean, by the rule of a frame without u_reset_flag
struct Count { uint32_t n; bool restart; };                   // n: entries in the mean; restart: the next entry starts a new mean
inline Count after_pass(Count c) { return {c.restart ? 1u : c.n + 1u, false}; }
// the same for an ordinary frame, whose u_reset_flag restarts the mean as well (render_batch)
inline Count after_frame(Count c, bool reset_flag) { return {(reset_flag || c.restart) ? 1u : c.n + 1u, false}; }
inline Count after_restart(Count c) { return {c.n, true}; }   // rtgl_clear_image, setting "aov", rtgl_adaptive_begin: the contents stay

// ---- the mesh hit of the camera rays
enum Stage { kStageNone = 0, kStageSolo = 1, kStageSplit = 2 };
// kStageNone: no triangle visits, guides_kernel<false> is the whole pass.  kStageSplit: option "kernel" 2, its intersect_kernel.
// kStageSolo: every other value of the option (0, 1 and 4), the matrix-core scan of kernel 4 with fresh keep bits.
inline Stage stage(int kernel_option, uint32_t tri_visits)
{
    if (tri_visits == 0u) return kStageNone;
    return kernel_option == kKernelSplit ? kStageSplit : kStageSolo;
}
// the value option "kernel" holds while the wave buffers of the pass are sized and its stage is launched
inline int stage_kernel(Stage s, int kernel_option) { return s == kStageSolo ? kKernelSolo : kernel_option; }
// launches of the pass, memsets not counted: ray generation (lean) + the stage + guides_kernel<true>, or guides_kernel<false> alone
inline bool generates_rays(Stage s) { return s != kStageNone; }
inline uint32_t blocks(uint32_t n0) { return (uint32_t)(((uint64_t)n0 + 255u) / 256u); }      // of guides_kernel and of ray generation
inline uint32_t wave_bounces() { return 1u; }                 // ensure_wave_buffers(n0, 1, false)
// an empty dispatch footprint (an image below 8 x 8, a tile without rows): nothing is enqueued, the count moves as for any pass
inline bool enqueues(uint32_t n0) { return n0 > 0u; }

// ---- what of a context the pass writes
enum Target {
    kPlanes, kPlanesCount, kFrameTimer,                       // written
    kWaveBuffers,                                             // scratch of the pass (queue 0, hit keys, scan buffers): rewritten by every frame before it reads them
    kImage, kSampleBuffers, kBucketBuffers, kRngStates, kCounters, kDenoised, kTemporal, kDisplay, kErrorSnapshot, kSessions, kRayEstimates, kKeptCameraBits,
    kTargets
};
inline bool writes(Target t) { return t == kPlanes || t == kPlanesCount || t == kFrameTimer || t == kWaveBuffers; }
// the kept camera bits (rt_camera_keep.hpp) are neither taken nor dropped: the scan of the pass culls into the per-frame bit buffer
inline bool takes_kept_bits() { return false; }
inline bool drops_kept_bits() { return false; }

}  // namespace rt_guides_plan

// The integer options of a context, in one table: the key of rtgl_set_option / rtgl_get_option, the environment's spelling that changes
// the default of a new context, the field, what may be done with it and the rule that refuses a value, next to the message it refuses
// with.  Plain host C++: no HIP and no environment access in this header, so that the host compiler can build it alone
// (tests/cpp/options_check.cpp); rtgl_amd.hip hands read_environment its getter.  A new option is a field of Options and a row of kRows.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace rt_options {

// (rtgl_amd.hip ties these to include/rtgl_amd.h, rt_wavefront.hpp and rt_mfma.hpp)
constexpr int kKernelMega = 0, kKernelRemoved3 = 3, kKernelSolo = 4, kAovAll = 15, kScalar = 0, kLds = 1;
constexpr int kBoundGroup = 64, kMaxChunk = 4096, kMfMaxChunkQuads = 32, kMfMaxGroupQuads = 64, kBatchMax = 16;

struct Options {
    int kernel = kKernelSolo;
    int rng_state = 0, counters = 0, kernel_timing = 0;
    int wf_rays = 4, wf_mode = kLds, wf_chunk = 256, wf_early = 0, wf_packed = 0;
    int mf_chunk_quads = 32, mf_group_quads = 32;      // (mf_group_quads: the value asked for; the context keeps the one in use)
    int cull = 3, sort_min_rays = 131072, scan_waves = 0, scan_dynamic = 0, frame_batch = 1;
    int debug_skip_exact = 0;      // timing diagnostics only, the image is wrong for 1 and 2.  1: survivors are dropped instead of tested; 2: broad phase rejects everything; 3: every segment through the list loop (image right)
    int aov = 0, denoise_source = 0, temporal_moments = 0, denoise_variance = 0;
    int camera_lean = 1;           // the lean camera bounce on frames that reuse the camera's keep bits (rt_wavefront.hpp, generate_rays_kernel)
    int shade_pass = 1;            // shade launches: 1 one pass where rt_shade_launch.hpp says so, 0 grid-stride passes everywhere
    int narrow_fused = 1;          // kernel 4: 1 the scan waves test their own survivors at their end (rt_scan.hpp, tail drain), 0 narrow_phase_kernel does
    int sort_move = 1;             // ray binning's move (rt_wavefront.hpp, WaveBuffers): 1 gathered by packet_cull_kernel, 0 scattered
};

// kSet: rtgl_set_option takes the key; kGet: rtgl_get_option answers it with the field; kBool: the stored value is value != 0
enum : unsigned { kSet = 1u, kGet = 2u, kBool = 4u };

struct Row {
    const char *key, *env;               // either may be NULL
    int Options::*field;
    unsigned flags;
    const char *(*refuse)(int value);    // the message a value is refused with, NULL where it is accepted; no function: every value is
};

#define RT_OPTION_RULE(accepted, message) [](int v) -> const char * { return (accepted) ? nullptr : message; }
constexpr Row kRows[] = {      // (internal linkage, the functions below too: the library exports nothing of this header)
    {"kernel", "RTGL_AMD_KERNEL", &Options::kernel, kSet | kGet, [](int v) -> const char * {
        return v == kKernelRemoved3 ? "kernel variant 3 (three waves per SIMD) was removed: it was not deterministic (DESIGN.md section 5); use 4" : v < kKernelMega || v > kKernelSolo ? "unknown kernel variant" : nullptr; }},
    {"wf_rays", nullptr, &Options::wf_rays, kSet | kGet, RT_OPTION_RULE(v == 1 || v == 2 || v == 4 || v == 8, "wf_rays must be 1, 2, 4 or 8")},
    {"wf_chunk", nullptr, &Options::wf_chunk, kSet | kGet, RT_OPTION_RULE(v >= kBoundGroup && v % kBoundGroup == 0 && v <= kMaxChunk, "wf_chunk must be a multiple of 64 in [64, 4096]")},
    {"debug_skip_exact", nullptr, &Options::debug_skip_exact, kSet, RT_OPTION_RULE(v >= 0 && v <= 3, "debug_skip_exact must be 0, 1, 2 or 3")},
    {"mf_chunk_quads", nullptr, &Options::mf_chunk_quads, kSet | kGet, RT_OPTION_RULE(v >= 1 && v <= kMfMaxChunkQuads, "mf_chunk_quads must be in [1, 32]")},
    {"scan_waves", "RTGL_AMD_SCAN_WAVES", &Options::scan_waves, kSet | kGet, RT_OPTION_RULE(v >= 0 && v <= 2, "scan_waves (waves per SIMD of the kernel-4 scan) must be 0 (default: two), 1 or 2")},
    {"scan_dynamic", "RTGL_AMD_SCAN_DYNAMIC", &Options::scan_dynamic, kSet | kGet, RT_OPTION_RULE(v >= 0 && v <= 4, "scan_dynamic must be 0 (chosen by the mesh), 1 (static turns), 2 (dynamic claims), 3 (planned: equal-cost intervals) or 4 (hybrid: turns + a claimed tail)")},
    {"narrow_fused", "RTGL_AMD_NARROW_FUSED", &Options::narrow_fused, kSet | kGet, RT_OPTION_RULE(v == 0 || v == 1, "narrow_fused must be 0 (narrow_phase_kernel tests the scan's survivors) or 1 (every scan wave tests its own at its end)")},
    {"camera_lean", "RTGL_AMD_CAMERA_LEAN", &Options::camera_lean, kSet | kGet, RT_OPTION_RULE(v == 0 || v == 1, "camera_lean must be 0 (camera rays travel through queue 0 in full) or 1 (shade rebuilds them while the camera's keep bits are reused)")},
    {"shade_pass", "RTGL_AMD_SHADE_PASS", &Options::shade_pass, kSet | kGet, RT_OPTION_RULE(v == 0 || v == 1, "shade_pass must be 0 (every shade launch in grid-stride passes) or 1 (one pass, a block per 256 slots of queue 0, unless the queue is expected to be all but empty)")},
    {"frame_batch", "RTGL_AMD_FRAME_BATCH", &Options::frame_batch, kSet | kGet, RT_OPTION_RULE(v >= 1 && v <= kBatchMax, "frame_batch (consecutive frames traced in one set of launches) must be 1..16")},
    {"cull", nullptr, &Options::cull, kSet | kGet, RT_OPTION_RULE(v >= 0 && v <= 3, "cull must be 0 (off), 1 (camera rays), 2 (every bounce, queues as they come) or 3 (camera rays + binned bounces)")},
    {"sort_min_rays", nullptr, &Options::sort_min_rays, kSet | kGet, RT_OPTION_RULE(v >= 0, "sort_min_rays (a bounce's queue is binned when at least this many rays are expected) must be >= 0")},
    {"mf_group_quads", nullptr, &Options::mf_group_quads, kSet, RT_OPTION_RULE(v >= 1 && v <= kMfMaxGroupQuads && !(v & (v - 1)), "mf_group_quads must be a power of two in [1, 64]")},      // (read: the value in use, by rtgl_get_option itself)
    {"wf_packed", nullptr, &Options::wf_packed, kSet | kGet | kBool, nullptr},
    {"wf_early", nullptr, &Options::wf_early, kSet | kGet, RT_OPTION_RULE(v >= 0, "wf_early is the number of leading bounces with the wave-level edge short circuit (>= 0)")},
    {"wf_mode", nullptr, &Options::wf_mode, kSet | kGet, RT_OPTION_RULE(v == kScalar || v == kLds, "wf_mode must be 0 (scalar) or 1 (lds)")},
    {"aov", nullptr, &Options::aov, kSet | kGet, RT_OPTION_RULE(v >= 0 && v <= kAovAll, "aov must be a mask of RTGL_AOV_ALBEDO | RTGL_AOV_NORMAL | RTGL_AOV_POSITION | RTGL_AOV_IDS (0: off)")},
    {"denoise_source", nullptr, &Options::denoise_source, kSet | kGet, RT_OPTION_RULE(v == 0 || v == 1, "denoise_source must be 0 (the accumulation image) or 1 (the latest history buffer of rtgl_temporal_accumulate)")},
    {"temporal_moments", nullptr, &Options::temporal_moments, kSet | kGet, RT_OPTION_RULE(v >= 0 && v <= 2, "temporal_moments must be 0 (off), 1 (luminance moments of the radiance) or 2 (of the radiance divided by the albedo)")},
    {"denoise_variance", nullptr, &Options::denoise_variance, kSet | kGet, RT_OPTION_RULE(v == 0 || v == 1, "denoise_variance must be 0 (the spatial estimate) or 1 (the temporal moments where the history is long enough)")},
    {"rng_state", nullptr, &Options::rng_state, kSet | kGet | kBool, nullptr},
    {"counters", nullptr, &Options::counters, kSet | kGet | kBool, nullptr},
    {"kernel_timing", nullptr, &Options::kernel_timing, kSet | kGet, RT_OPTION_RULE(v >= 0, "kernel_timing must be 0 (off) or the sampling period in frames")},
    {nullptr, "RTGL_AMD_SORT_MOVE", &Options::sort_move, 0u, RT_OPTION_RULE(v == 0 || v == 1, "sort_move must be 0 or 1")},      // (A/B of ray binning's move: the environment only)
};
#undef RT_OPTION_RULE
constexpr unsigned kRowCount = sizeof(kRows) / sizeof(kRows[0]);
static_assert(kRowCount <= 32u, "read_environment reports the rows it set in 32 bits");

// the row of a key, NULL where no row has it
static inline const Row *find(const char *key)
{
    for (const Row &row : kRows) if (row.key && !strcmp(row.key, key)) return &row;
    return nullptr;
}

// the message `value` is refused with, NULL where the row takes it
static inline const char *refusal(const Row &row, int value) { return row.refuse ? row.refuse(value) : nullptr; }

// NULL: `value` was stored; otherwise the message it is refused with, and nothing changed
static inline const char *set(Options &opt, const Row &row, int value)
{
    if (const char *message = refusal(row, value)) return message;
    opt.*row.field = row.flags & kBool ? value != 0 : value;
    return nullptr;
}

// the bit of a field's row in what read_environment returns
static constexpr uint32_t row_bit(int Options::*field, unsigned i = 0) { return i == kRowCount ? 0u : kRows[i].field == field ? 1u << i : row_bit(field, i + 1); }

// The environment's spellings change the defaults of a new context: a variable that is set is read as atoi reads it, and kept where the
// row's rule accepts the number (a refused one is passed over in silence).  Returns the rows that were set.
static inline uint32_t read_environment(Options &opt, const char *(*getter)(const char *))
{
    uint32_t rows = 0;
    for (unsigned i = 0; i < kRowCount; ++i)
        if (const char *text = kRows[i].env ? getter(kRows[i].env) : nullptr)
            if (!set(opt, kRows[i], atoi(text))) rows |= 1u << i;
    return rows;
}

}      // namespace rt_options

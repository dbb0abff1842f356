// rt_tonemap.hpp -- rtgl_tonemap: the display transform behind the float buffers.  A luminance histogram of the source, an integer solve
// for the exposure that stays on the device, a tone curve and the sRGB encoding to RGBA8.  The contract is in include/rtgl_amd.h
// ("display transform"), the reasoning in DESIGN.md 5.9.  No reference counterpart: the reference's only way to 8 bits is the clamp of
// glGetTexImage (image_to_u8_kernel, rtgl_amd.hip), which stays as it is.
//
// Nothing here needs a transcendental function: the bin of a luminance is a shift of its bits, the exposure is one multiply by a table
// entry and an exact power of two, the sRGB code is a count of thresholds.  The float arithmetic is defined operation by operation like
// the denoisers' (binary32, one rounding each, no contraction, correctly rounded divide), the integer arithmetic is exact and its sums
// commute, so that the numpy restatement (tests/tonemap_mirror.py) gives the same bits whatever the order of the blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.hpp"
#include "rt_wavefront.hpp"

#pragma clang fp contract(off)

namespace rt {

// P[r] = float32(2^(-r/64)): the fraction of the exposure's binary logarithm.  THE COMMITTED VALUES ARE THE CONTRACT.
__device__ const float kTonemapExposure[64] = {
    0x1.000000p+0f, 0x1.fa7c18p-1f, 0x1.f50766p-1f, 0x1.efa1bep-1f, 0x1.ea4afap-1f, 0x1.e502eep-1f, 0x1.dfc974p-1f, 0x1.da9e60p-1f,
    0x1.d5818ep-1f, 0x1.d072d4p-1f, 0x1.cb720ep-1f, 0x1.c67f12p-1f, 0x1.c199bep-1f, 0x1.bcc1eap-1f, 0x1.b7f770p-1f, 0x1.b33a2cp-1f,
    0x1.ae89fap-1f, 0x1.a9e6b6p-1f, 0x1.a5503cp-1f, 0x1.a0c668p-1f, 0x1.9c4918p-1f, 0x1.97d82ap-1f, 0x1.93737cp-1f, 0x1.8f1aeap-1f,
    0x1.8ace54p-1f, 0x1.868d9ap-1f, 0x1.82589ap-1f, 0x1.7e2f34p-1f, 0x1.7a1148p-1f, 0x1.75feb6p-1f, 0x1.71f75ep-1f, 0x1.6dfb24p-1f,
    0x1.6a09e6p-1f, 0x1.662388p-1f, 0x1.6247ecp-1f, 0x1.5e76f2p-1f, 0x1.5ab07ep-1f, 0x1.56f474p-1f, 0x1.5342b6p-1f, 0x1.4f9b28p-1f,
    0x1.4bfdaep-1f, 0x1.486a2cp-1f, 0x1.44e086p-1f, 0x1.4160a2p-1f, 0x1.3dea64p-1f, 0x1.3a7db4p-1f, 0x1.371a74p-1f, 0x1.33c08cp-1f,
    0x1.306fe0p-1f, 0x1.2d285ap-1f, 0x1.29e9e0p-1f, 0x1.26b456p-1f, 0x1.2387a6p-1f, 0x1.2063b8p-1f, 0x1.1d4874p-1f, 0x1.1a35bep-1f,
    0x1.172b84p-1f, 0x1.1429aap-1f, 0x1.11301ep-1f, 0x1.0e3ec4p-1f, 0x1.0b5586p-1f, 0x1.087452p-1f, 0x1.059b0ep-1f, 0x1.02c9a4p-1f,
};

// T[k], k = 1..255 = float32 of the sRGB-decoded (k - 0.5) / 255 (IEC 61966-2-1, evaluated in float64): a linear value y has the code
// k exactly if T[k] <= y < T[k + 1].  T[0] is never compared.  THE COMMITTED VALUES ARE THE CONTRACT.
__device__ const float kTonemapThreshold[256] = {
    0x0.000000p+0f, 0x1.3e4568p-13f, 0x1.dd681cp-12f, 0x1.8dd6c2p-11f, 0x1.167cbap-10f, 0x1.660e14p-10f, 0x1.b59f6ep-10f, 0x1.029864p-9f,
    0x1.2a6112p-9f, 0x1.5229bep-9f, 0x1.79f26ap-9f, 0x1.a1e5a0p-9f, 0x1.cbf734p-9f, 0x1.f86806p-9f, 0x1.13a0bep-8f, 0x1.2c4666p-8f,
    0x1.46297ap-8f, 0x1.614e60p-8f, 0x1.7db96cp-8f, 0x1.9b6edap-8f, 0x1.ba72cep-8f, 0x1.dac95ep-8f, 0x1.fc768ap-8f, 0x1.0fbf22p-7f,
    0x1.21f234p-7f, 0x1.34d662p-7f, 0x1.486d8ep-7f, 0x1.5cb98ep-7f, 0x1.71bc32p-7f, 0x1.877748p-7f, 0x1.9dec90p-7f, 0x1.b51dc8p-7f,
    0x1.cd0ca8p-7f, 0x1.e5bae0p-7f, 0x1.ff2a1ep-7f, 0x1.0cae04p-6f, 0x1.1a291cp-6f, 0x1.28072ap-6f, 0x1.3648f6p-6f, 0x1.44ef4cp-6f,
    0x1.53faeep-6f, 0x1.636ca4p-6f, 0x1.734530p-6f, 0x1.838550p-6f, 0x1.942dc4p-6f, 0x1.a53f48p-6f, 0x1.b6ba94p-6f, 0x1.c8a062p-6f,
    0x1.daf168p-6f, 0x1.edae5cp-6f, 0x1.006bf6p-5f, 0x1.0a3768p-5f, 0x1.1439d8p-5f, 0x1.1e73a0p-5f, 0x1.28e514p-5f, 0x1.338e8ap-5f,
    0x1.3e7056p-5f, 0x1.498acep-5f, 0x1.54de42p-5f, 0x1.606b08p-5f, 0x1.6c316ep-5f, 0x1.7831c6p-5f, 0x1.846c62p-5f, 0x1.90e192p-5f,
    0x1.9d91a4p-5f, 0x1.aa7ce4p-5f, 0x1.b7a3a4p-5f, 0x1.c50630p-5f, 0x1.d2a4d4p-5f, 0x1.e07fdcp-5f, 0x1.ee9794p-5f, 0x1.fcec46p-5f,
    0x1.05bf20p-4f, 0x1.0d26e4p-4f, 0x1.14ad94p-4f, 0x1.1c5356p-4f, 0x1.24184cp-4f, 0x1.2bfc9cp-4f, 0x1.34006ap-4f, 0x1.3c23d6p-4f,
    0x1.446708p-4f, 0x1.4cca1ep-4f, 0x1.554d40p-4f, 0x1.5df08ep-4f, 0x1.66b428p-4f, 0x1.6f9836p-4f, 0x1.789cd4p-4f, 0x1.81c228p-4f,
    0x1.8b0850p-4f, 0x1.946f72p-4f, 0x1.9df7aap-4f, 0x1.a7a11cp-4f, 0x1.b16beap-4f, 0x1.bb5830p-4f, 0x1.c56612p-4f, 0x1.cf95b0p-4f,
    0x1.d9e72ap-4f, 0x1.e45a9ep-4f, 0x1.eef02ep-4f, 0x1.f9a7f8p-4f, 0x1.02410ep-3f, 0x1.07bf5cp-3f, 0x1.0d4ef6p-3f, 0x1.12efecp-3f,
    0x1.18a24cp-3f, 0x1.1e6626p-3f, 0x1.243b8ap-3f, 0x1.2a2286p-3f, 0x1.301b2ap-3f, 0x1.362582p-3f, 0x1.3c41a2p-3f, 0x1.426f94p-3f,
    0x1.48af6ap-3f, 0x1.4f0132p-3f, 0x1.5564f8p-3f, 0x1.5bdacep-3f, 0x1.6262c0p-3f, 0x1.68fce0p-3f, 0x1.6fa938p-3f, 0x1.7667d8p-3f,
    0x1.7d38cep-3f, 0x1.841c28p-3f, 0x1.8b11f6p-3f, 0x1.921a42p-3f, 0x1.99351ep-3f, 0x1.a06296p-3f, 0x1.a7a2bap-3f, 0x1.aef594p-3f,
    0x1.b65b34p-3f, 0x1.bdd3a6p-3f, 0x1.c55efap-3f, 0x1.ccfd3ep-3f, 0x1.d4ae7cp-3f, 0x1.dc72c2p-3f, 0x1.e44a20p-3f, 0x1.ec34a4p-3f,
    0x1.f43256p-3f, 0x1.fc4348p-3f, 0x1.0233c2p-2f, 0x1.064f8ep-2f, 0x1.0a750cp-2f, 0x1.0ea442p-2f, 0x1.12dd3ap-2f, 0x1.171ff8p-2f,
    0x1.1b6c82p-2f, 0x1.1fc2dep-2f, 0x1.242316p-2f, 0x1.288d2cp-2f, 0x1.2d0128p-2f, 0x1.317f12p-2f, 0x1.3606eep-2f, 0x1.3a98c2p-2f,
    0x1.3f3496p-2f, 0x1.43da70p-2f, 0x1.488a54p-2f, 0x1.4d444cp-2f, 0x1.52085ap-2f, 0x1.56d688p-2f, 0x1.5baed8p-2f, 0x1.609154p-2f,
    0x1.657e00p-2f, 0x1.6a74e2p-2f, 0x1.6f7600p-2f, 0x1.748160p-2f, 0x1.79970ap-2f, 0x1.7eb700p-2f, 0x1.83e14cp-2f, 0x1.8915f2p-2f,
    0x1.8e54f8p-2f, 0x1.939e64p-2f, 0x1.98f23ap-2f, 0x1.9e5084p-2f, 0x1.a3b944p-2f, 0x1.a92c80p-2f, 0x1.aeaa42p-2f, 0x1.b4328ap-2f,
    0x1.b9c562p-2f, 0x1.bf62cep-2f, 0x1.c50ad4p-2f, 0x1.cabd7ap-2f, 0x1.d07ac4p-2f, 0x1.d642bap-2f, 0x1.dc1560p-2f, 0x1.e1f2bcp-2f,
    0x1.e7dad4p-2f, 0x1.edcdaep-2f, 0x1.f3cb4ep-2f, 0x1.f9d3bcp-2f, 0x1.ffe6fap-2f, 0x1.030288p-1f, 0x1.061702p-1f, 0x1.0930eep-1f,
    0x1.0c504cp-1f, 0x1.0f7522p-1f, 0x1.129f72p-1f, 0x1.15cf3ep-1f, 0x1.190488p-1f, 0x1.1c3f54p-1f, 0x1.1f7fa4p-1f, 0x1.22c57ap-1f,
    0x1.2610dap-1f, 0x1.2961c8p-1f, 0x1.2cb844p-1f, 0x1.301450p-1f, 0x1.3375f2p-1f, 0x1.36dd2ap-1f, 0x1.3a49fcp-1f, 0x1.3dbc6ap-1f,
    0x1.413476p-1f, 0x1.44b224p-1f, 0x1.483576p-1f, 0x1.4bbe6ep-1f, 0x1.4f4d10p-1f, 0x1.52e15ep-1f, 0x1.567b58p-1f, 0x1.5a1b04p-1f,
    0x1.5dc064p-1f, 0x1.616b7ap-1f, 0x1.651c46p-1f, 0x1.68d2d0p-1f, 0x1.6c8f16p-1f, 0x1.70511cp-1f, 0x1.7418e6p-1f, 0x1.77e672p-1f,
    0x1.7bb9c8p-1f, 0x1.7f92e8p-1f, 0x1.8371d4p-1f, 0x1.875690p-1f, 0x1.8b411cp-1f, 0x1.8f317cp-1f, 0x1.9327b4p-1f, 0x1.9723c4p-1f,
    0x1.9b25b0p-1f, 0x1.9f2d7ap-1f, 0x1.a33b22p-1f, 0x1.a74eb0p-1f, 0x1.ab6820p-1f, 0x1.af877ap-1f, 0x1.b3acbep-1f, 0x1.b7d7ecp-1f,
    0x1.bc090cp-1f, 0x1.c0401ap-1f, 0x1.c47d1ep-1f, 0x1.c8c018p-1f, 0x1.cd090ap-1f, 0x1.d157f6p-1f, 0x1.d5ace0p-1f, 0x1.da07c8p-1f,
    0x1.de68b4p-1f, 0x1.e2cfa2p-1f, 0x1.e73c98p-1f, 0x1.ebaf98p-1f, 0x1.f028a2p-1f, 0x1.f4a7bap-1f, 0x1.f92ce2p-1f, 0x1.fdb81cp-1f,
};

// One histogram set: 256 bins and, in word 256, the pixels that do not count.  The state buffer of a context holds two sets that take
// turns (the solve of a call zeroes the set the next call counts in, as the bin counters of the ray binning do: no fill launch) and the
// exposure behind them.
constexpr int kToneBins = 256, kToneWords = kToneBins + 1;
constexpr int kToneExposureWord = 2 * kToneWords, kToneStateWords = kToneExposureWord + 2;
constexpr int kToneBinBias = 888;                                      // (127 - 16) * 8: bin 0 begins at 2^-16, eight bins per binade

__device__ __forceinline__ float tonemap_lum(float r, float g, float b) { return (0.25f * r + 0.5f * g) + 0.25f * b; }
__device__ __forceinline__ uint32_t tonemap_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Grid-stride over the pixels, one 16-byte load per lane and step.  Every wave counts into a histogram of its own in LDS (4 x 257 words,
// 4112 bytes) with LDS integer adds; the pixels that do not count are summed in a register first.  At the end lane t sums bin t over the
// four waves and adds it to the global set with one integer add whose result nobody waits for, bins that stayed empty not at all.
__global__ void __launch_bounds__(256) tonemap_histogram_kernel(const float4 *__restrict__ src, size_t n, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[4 * kToneWords];
    const int tid = (int)threadIdx.x;
    uint32_t *mine = h + (tid >> 6) * kToneWords;
    for (int e = tid; e < 4 * kToneWords; e += 256) h[e] = 0u;
    __syncthreads();
    uint32_t ignored = 0u;
    for (size_t i = (size_t)blockIdx.x * 256u + (size_t)tid; i < n; i += (size_t)gridDim.x * 256u) {
        const float4 c = src[i];
        const float L = tonemap_lum(c.x, c.y, c.z);
        if (L > 0.0f) {                                                // (NaN, +-0 and negatives do not count)
            int b = (int)(__float_as_uint(L) >> 20) - kToneBinBias;
            b = b < 0 ? 0 : (b > kToneBins - 1 ? kToneBins - 1 : b);
            atomicAdd(mine + b, 1u);
        } else ++ignored;
    }
    if (ignored) atomicAdd(mine + kToneBins, ignored);
    __syncthreads();
    for (int e = tid; e < kToneWords; e += 256) {
        const uint32_t s = (h[e] + h[kToneWords + e]) + (h[2 * kToneWords + e] + h[3 * kToneWords + e]);
        if (s) atomicAdd(hist + e, s);
    }
}

struct TonemapSolveArgs {
    uint32_t *state;                      // two histogram sets and the exposure (kToneStateWords words)
    int32_t set;                          // the set this call counted in; the other one is zeroed for the next call
    uint32_t use_prev;                    // an exposure stored since the last reset is in the state
    uint32_t low_permille, high_permille;
    float exposure, key, adapt, exposure_min, exposure_max;
};

// One wave.  Lane l owns bins 4 l .. 4 l + 3: a scan over the lanes gives the pixels below its bins, from which it clips its bins to the
// kept range [lo, N - hi) of the ordered pixels; K and S are summed over the lanes and lane 0 does the rest.  All in 64-bit integers.
__global__ void __launch_bounds__(64) tonemap_solve_kernel(TonemapSolveArgs a)
{
    const int lane = (int)threadIdx.x;
    const uint32_t *cur = a.state + a.set * kToneWords;
    uint32_t *next = a.state + (a.set ^ 1) * kToneWords;
    for (int e = lane; e < kToneWords; e += 64) store_through(next + e, 0u);
    unsigned long long hb[4], own = 0ull;
#pragma unroll
    for (int k = 0; k < 4; ++k) { hb[k] = tonemap_load(cur + 4 * lane + k); own += hb[k]; }
    unsigned long long inc = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(inc, (unsigned)d);
        if (lane >= d) inc += t;
    }
    const long long N = (long long)__shfl(inc, 63);
    const long long lo = N * (long long)a.low_permille / 1000, top = N - N * (long long)a.high_permille / 1000;
    long long c = (long long)(inc - own), K = 0, S = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long hi_end = (c + (long long)hb[k] < top) ? c + (long long)hb[k] : top, lo_end = (c > lo) ? c : lo;
        const long long kept = hi_end > lo_end ? hi_end - lo_end : 0;
        K += kept;
        S += kept * (long long)(2 * (4 * lane + k) + 1);
        c += (long long)hb[k];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { K += __shfl_xor(K, d); S += __shfl_xor(S, d); }
    if (lane != 0) return;
    float target = a.exposure;                                         // no pixel counts
    if (N > 0) {
        const unsigned long long m = (unsigned long long)(4 * S) / (unsigned long long)K;          // K >= 1: low + high < 1000; m <= 2044
        const uint32_t q = (uint32_t)m >> 6, r = (uint32_t)m & 63u;
        // ldexp(key P[r], 16 - q): the multiply by an exact power of two rounds once, as ldexp does
        target = (a.key * kTonemapExposure[r]) * __uint_as_float((127u + 16u - q) << 23);
    }
    float e = target;
    if (a.use_prev && a.adapt < 1.0f) {
        const float prev = __uint_as_float(tonemap_load(a.state + kToneExposureWord));
        e = prev + (target - prev) * a.adapt;
    }
    e = (e < a.exposure_min) ? a.exposure_min : e;
    e = (e > a.exposure_max) ? a.exposure_max : e;
    store_through(a.state + kToneExposureWord, __float_as_uint(e));
}

struct TonemapMapArgs {
    const float4 *src;
    uint32_t *display;                    // RGBA8, one word per pixel, rows in the source's order
    const uint32_t *exposure_word;        // auto: where the solve left the exposure; NULL: `exposure`
    size_t n;
    float exposure, white2;               // white2 = white white
};

// the sRGB code of y: the number of thresholds T[1..255] that are <= y, by an 8-step binary search (a NaN compares false: 0)
__device__ __forceinline__ uint32_t tonemap_encode(const float *T, float y)
{
    uint32_t k = 0u;
#pragma unroll
    for (uint32_t s = 128u; s; s >>= 1) k += (T[k + s] <= y) ? s : 0u;      // (k + s is 1..255)
    return k;
}

// Grid-stride over the pixels: one 16-byte load and one 4-byte store per pixel, the 256 thresholds in LDS (1 KB).  kOp: 0 linear,
// 1 Reinhard with white point (on the luminance, the colour scaled), 2 the ACES fit per channel.
template <int kOp>
__global__ void __launch_bounds__(256) tonemap_map_kernel(TonemapMapArgs a)
{
    __shared__ float T[256];
    const int tid = (int)threadIdx.x;
    T[tid] = kTonemapThreshold[tid];
    __syncthreads();
    const float e = a.exposure_word ? __uint_as_float(tonemap_load(a.exposure_word)) : a.exposure;
    for (size_t i = (size_t)blockIdx.x * 256u + (size_t)tid; i < a.n; i += (size_t)gridDim.x * 256u) {
        const float4 c = a.src[i];
        const float xr = c.x * e, xg = c.y * e, xb = c.z * e;
        float yr = xr, yg = xg, yb = xb;
        if constexpr (kOp == 1) {
            const float Lx = tonemap_lum(xr, xg, xb);
            const float s = (1.0f + Lx / a.white2) / (1.0f + Lx);
            yr = xr * s; yg = xg * s; yb = xb * s;
        }
        if constexpr (kOp == 2) {
            auto fit = [](float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); };
            yr = fit(xr); yg = fit(xg); yb = fit(xb);
        }
        const uint32_t px = tonemap_encode(T, yr) | (tonemap_encode(T, yg) << 8) | (tonemap_encode(T, yb) << 16) | 0xff000000u;
        store_through(a.display + i, px);                              // (rewritten by every call: rt_wavefront.hpp, store_through)
    }
}

}  // namespace rt

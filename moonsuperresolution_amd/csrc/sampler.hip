// sampler.hip — counter-based sampler noise (msr_sampler_noise; the recipe is stated in include/moonsr.h and is part of the ABI).
//
// eps[b][4g .. 4g+3] is a pure function of (seed, row id, g): one Philox4x32-10 block per thread, counter (g, id0, id1, id2),
// key (seed lo, seed hi), then two Box-Muller pairs.  Everything after the integer block is fp32 + - * /, sqrtf and integer
// operations in a fixed order (the tree is built with -ffp-contract=off), so the NumPy twin (ops.sampler_noise) reproduces it
// bit for bit: no libm, no fast-math intrinsic.
//   * log(u): the exponent comes from a count-leading-zeros of the integer, the mantissa m in [sqrt(1/2), sqrt(2)) goes through
//     2 atanh(s), s = (m - 1) / (m + 1), |s| <= 0.1716, as an odd polynomial up to s^9 (truncation < 3e-9 relative).
//   * sin / cos: the octant is the top three bits of the integer, odd octants mirror the remaining bits, and the angle in
//     (0, pi/4) goes through the Taylor polynomials up to x^9 / x^10 (truncation < 2e-9).
// One thread per block of four values, one 16-byte vector store each, the tail of the grid guarded.  No atomics, no LDS.
#include "host.h"

namespace msr {

namespace {

constexpr int kThreads = 256;

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = U4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// sqrt(-2 ln u), u = (n + 0.5) / 2^32 in (0, 1)
__device__ __forceinline__ float radius(uint32_t n) {
    const int lz = n ? __builtin_clz(n) : 32;
    // 2n + 1 has 33 - lz significant bits; its top 24 are the mantissa t / 2^23 in [1, 2), and u = (t / 2^23) * 2^(-1 - lz)
    const uint32_t t = (uint32_t)(((((uint64_t)n << 1) | 1u) << lz) >> 9);
    float m = (float)t * 1.1920928955078125e-07f;           // 2^-23: exact
    int e = -1 - lz;
    if (t >= 0xB504F4u) { m = m * 0.5f; e += 1; }           // m >= sqrt(2) (as 24 bits): halve, so that m is in [0.7071, 1.4142)
    const float s = (m - 1.0f) / (m + 1.0f);
    const float s2 = s * s;
    float p = 0x1.c71c72p-4f;                               // 1/9
    p = p * s2 + 0x1.24924ap-3f;                            // 1/7
    p = p * s2 + 0x1.99999ap-3f;                            // 1/5
    p = p * s2 + 0x1.555556p-2f;                            // 1/3
    p = p * s2 + 1.0f;
    const float lnm = (s + s) * p;                          // ln m = 2 atanh(s)
    const float ln = (float)e * 0x1.62e43p-1f + lnm;        // ln u < 0
    return sqrtf(-2.0f * ln);
}

// (cos, sin) of 2 pi (n + 0.5) / 2^32
__device__ __forceinline__ void cos_sin(uint32_t n, float& c, float& s) {
    const uint32_t oct = n >> 29;
    uint32_t f = n & 0x1FFFFFFFu;
    if (oct & 1u) f = 0x1FFFFFFFu - f;                      // odd octants run backwards: pi/4 - angle
    const float a = (float)(((f >> 6) << 1) | 1u) * 5.9604644775390625e-08f;   // (2k + 1) / 2^24 in (0, 1): exact
    const float x = a * 0x1.921fb6p-1f;                     // pi/4
    const float x2 = x * x;
    float ps = 0x1.71de3ap-19f;                             // 1/9!
    ps = ps * x2 - 0x1.a01a02p-13f;                         // 1/7!
    ps = ps * x2 + 0x1.111112p-7f;                          // 1/5!
    ps = ps * x2 - 0x1.555556p-3f;                          // 1/3!
    const float sn = x + x * (x2 * ps);
    float pc = -0x1.27e4fcp-22f;                            // 1/10!
    pc = pc * x2 + 0x1.a01a02p-16f;                         // 1/8!
    pc = pc * x2 - 0x1.6c16c2p-10f;                         // 1/6!
    pc = pc * x2 + 0x1.555556p-5f;                          // 1/4!
    pc = pc * x2 - 0.5f;
    const float cs = 1.0f + x2 * pc;
    const bool swap = ((oct + 1u) >> 1) & 1u;               // octants 1, 2, 5, 6
    c = swap ? sn : cs;
    s = swap ? cs : sn;
    if (((oct + 2u) >> 2) & 1u) c = -c;                     // octants 2 .. 5
    if (oct >> 2) s = -s;                                   // octants 4 .. 7
}

__global__ __launch_bounds__(kThreads) void sampler_noise_kernel(uint32_t k0, uint32_t k1, const uint32_t* __restrict__ ids,
                                                                uint32_t first_row, float* __restrict__ eps, uint32_t n_blocks,
                                                                uint32_t groups) {
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= n_blocks) return;
    const uint32_t b = i / groups, g = i - b * groups;
    U4 c{g, first_row + b, 0u, 0u};
    if (ids) { const uint32_t* id = ids + (size_t)b * 3; c.y = id[0]; c.z = id[1]; c.w = id[2]; }
    const U4 w = philox4x32_10(c, k0, k1);
    float c0, s0, c1, s1;
    cos_sin(w.y, c0, s0);
    cos_sin(w.w, c1, s1);
    const float r0 = radius(w.x), r1 = radius(w.z);
    reinterpret_cast<float4*>(eps)[i] = make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
}

}  // namespace

}  // namespace msr

using namespace msr;

extern "C" {

int msr_sampler_noise(msr_handle* h, uint64_t seed, const uint32_t* ids_dev, uint32_t first_row, float* eps_dev, int32_t B,
                      int32_t L, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!eps_dev || B < 1 || L < 4 || L % 4 || (int64_t)B * L >= ((int64_t)1 << 33) || ((uintptr_t)eps_dev & 15))
        return fail(h, MSR_ERR_INVALID, "msr_sampler_noise: bad argument (B >= 1, L a positive multiple of 4, B * L / 4 < 2^31, "
                    "eps_dev aligned to 16 bytes)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const uint32_t groups = (uint32_t)(L / 4), n_blocks = (uint32_t)B * groups;
    const uint32_t grid = (n_blocks + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(sampler_noise_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, (uint32_t)(seed & 0xFFFFFFFFu),
                       (uint32_t)(seed >> 32), ids_dev, first_row, eps_dev, n_blocks, groups);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, MSR_ERR_DEVICE, "launch of sampler_noise failed: %s", hipGetErrorString(e));
    return MSR_OK;
}

}  // extern "C"

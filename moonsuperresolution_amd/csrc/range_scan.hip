// range_scan.hip — activation-range scan of the narrow activation images ("range scan").
//
// One memory-bound launch walks a small device table of activation tensors and leaves, per tensor, a record
//   { max |hi| (bits of the fp32 value), interior elements, cross-piece clipped, clamped, non-finite }
// for the formats whose pieces have a finite range (the planner's out_split, kernels.h OutFormat): OUT_F16X2, OUT_BF8, OUT_F16C, OUT_F16C6.
//
//  * Only the MAIN piece is read.  In the three chunk formats it is the first 64 bytes (32 fp16) of every 128-byte chunk; an
//    e4m3 cross piece of the f16c image clips exactly when |hi| > 464 (the largest value that still rounds to 448), so the
//    count is taken on hi as well.  bf8 tensors are their own main piece.
//  * Magnitudes are compared on the integer bit pattern (fp16 and bf8 are monotonic in their bits): no conversions, except the
//    one that turns a workgroup's maximum into fp32 bits for the atomic.
//  * 16-byte loads only.  A workgroup takes whole interior rows (b, y) of a tensor — a row is one contiguous run of chunks,
//    so the zero border is never read and never counted — and its threads stride over the row.
//  * A 16-byte item whose largest magnitude is below every threshold (the normal case) costs a few packed max operations; only
//    an item that holds a flagged value is looked at element by element.
//  * Reduction: __shfl_xor inside the wave, LDS across the four waves, then ONE lane issues one vector atomicMax and up to four
//    64-bit vector atomicAdds into the tensor's record.  Max and integer sums are order-independent: the result is deterministic.
//  * The grid is persistent: a fixed number of workgroups per CU, each looping over every table entry.
#include "kernels.h"

namespace msr {

namespace {

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ us2 as_us2(unsigned w) { return __builtin_bit_cast(us2, w); }
__device__ __forceinline__ us2 max2(us2 a, us2 b) { return __builtin_elementwise_max(a, b); }

struct Acc {
    unsigned mx;          // largest finite magnitude, as fp16 bits (bf8: byte << 8)
    unsigned total, cross, clamped, nonfinite;
};

// One 16-byte item of fp16 main pieces: 8 magnitudes.  `fast` = the largest bit pattern that raises no count.
__device__ __forceinline__ void scan_item_f16(const uint4 v, unsigned fast, unsigned cross_thr, us2& mxv, Acc& a) {
    const unsigned w[4] = {v.x & 0x7fff7fffu, v.y & 0x7fff7fffu, v.z & 0x7fff7fffu, v.w & 0x7fff7fffu};
    const us2 m = max2(max2(as_us2(w[0]), as_us2(w[1])), max2(as_us2(w[2]), as_us2(w[3])));
    const unsigned top = m.x > m.y ? m.x : m.y;
    if (top <= fast) {
        mxv = max2(mxv, m);
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int hlf = 0; hlf < 2; ++hlf) {
            const unsigned e = (w[k] >> (16 * hlf)) & 0xffffu;
            if (e < 0x7c00u) a.mx = a.mx > e ? a.mx : e;
            else a.nonfinite += 1;
            a.clamped += e == 0x7bffu;
            a.cross += e > cross_thr;
        }
}

// One 16-byte item of bf8 (e5m2) bytes: 16 magnitudes; a byte is the high byte of the fp16 with the same value.
__device__ __forceinline__ void scan_item_bf8(const uint4 v, us2& mxv, Acc& a) {
    const unsigned w[4] = {v.x & 0x7f7f7f7fu, v.y & 0x7f7f7f7fu, v.z & 0x7f7f7f7fu, v.w & 0x7f7f7f7fu};
    us2 m = as_us2(0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) m = max2(m, max2(as_us2(w[k] & 0x00ff00ffu), as_us2((w[k] >> 8) & 0x00ff00ffu)));
    const unsigned top = m.x > m.y ? m.x : m.y;
    if (top < 0x7bu) {
        mxv = max2(mxv, as_us2(__builtin_bit_cast(unsigned, m) << 8));
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned e = (w[k] >> (8 * q)) & 0xffu;
            if (e < 0x7cu) a.mx = a.mx > (e << 8) ? a.mx : (e << 8);
            else a.nonfinite += 1;
            a.clamped += e == 0x7bu;
        }
}

// bits of a finite, non-negative fp16 -> bits of the fp32 with the same value
__device__ __forceinline__ unsigned f16_bits_to_f32_bits(unsigned hb) {
    if (hb >= 0x400u) return (((hb >> 10) + 112u) << 23) | ((hb & 0x3ffu) << 13);
    return __float_as_uint((float)hb * 5.9604644775390625e-8f);     // subnormal: mantissa * 2^-24, exact
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)v, o); v = v > t ? v : t; }
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void range_scan_kernel(const RangeScanItem* __restrict__ table, int n_items,
                                                              RangeScanRecord* __restrict__ rec) {
    __shared__ unsigned red[kThreads / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = 0; t < n_items; ++t) {
        const RangeScanItem it = table[t];
        const int rows = it.B * it.r;
        if ((int)blockIdx.x >= rows) continue;                     // uniform over the workgroup: nothing of this tensor is ours
        const bool bytes = it.format == OUT_BF8;
        // 16-byte items per interior row: four per 128-byte chunk (the fp16 main piece), or the whole run of bf8 bytes
        const int per_row = bytes ? it.r * (it.px_bytes >> 4) : it.r * (it.C >> 5) * 4;
        const unsigned fast = it.format == OUT_F16C ? 0x5f40u : 0x7bfeu;  // 464 | the value below 65504
        const unsigned cross_thr = it.format == OUT_F16C ? 0x5f40u : 0xffffu;
        const bool pad_ch = bytes && it.px_bytes != it.C;          // bf8 pixels padded with zero channels: not counted
        Acc a{0u, 0u, 0u, 0u, 0u};
        us2 mxv = as_us2(0u);
        for (int row = blockIdx.x; row < rows; row += gridDim.x) {
            const int b = row / it.r, y = row - b * it.r;
            const size_t px = it.padded ? ((size_t)(b * (it.r + 2) + y + 1) * (it.r + 2) + 1) : (size_t)row * it.r;
            const uint4* p = reinterpret_cast<const uint4*>(static_cast<const char*>(it.base) + px * (size_t)it.px_bytes);
            if (bytes) {
#pragma unroll 4
                for (int j = tid; j < per_row; j += kThreads) {
                    scan_item_bf8(p[j], mxv, a);
                    if (pad_ch) a.total += ((unsigned)(j << 4) % (unsigned)it.px_bytes) < (unsigned)it.C ? 16u : 0u;
                }
                if (!pad_ch) a.total += tid < per_row ? (unsigned)((per_row - tid + kThreads - 1) / kThreads) * 16u : 0u;
            } else {
#pragma unroll 4
                for (int j = tid; j < per_row; j += kThreads)
                    scan_item_f16(p[(size_t)(j >> 2) * 8 + (j & 3)], fast, cross_thr, mxv, a);
                a.total += tid < per_row ? (unsigned)((per_row - tid + kThreads - 1) / kThreads) * 8u : 0u;
            }
        }
        unsigned m = mxv.x > mxv.y ? mxv.x : mxv.y;
        m = m > a.mx ? m : a.mx;
        const unsigned v[5] = {wave_max(m), wave_sum(a.total), wave_sum(a.cross), wave_sum(a.clamped), wave_sum(a.nonfinite)};
        __syncthreads();                                           // the previous tensor's read of `red` is over
        if (lane == 0)
#pragma unroll
            for (int k = 0; k < 5; ++k) red[wave][k] = v[k];
        __syncthreads();
        if (tid == 0) {
            unsigned s[5] = {red[0][0], red[0][1], red[0][2], red[0][3], red[0][4]};
#pragma unroll
            for (int w = 1; w < kThreads / 64; ++w) {
                s[0] = s[0] > red[w][0] ? s[0] : red[w][0];
#pragma unroll
                for (int k = 1; k < 5; ++k) s[k] += red[w][k];
            }
            RangeScanRecord* r = rec + it.record;
            // fp16 bits -> fp32 bits of the same (finite, non-negative) value: positive floats are ordered like their bits
            if (s[0]) atomicMax(&r->max_abs_bits, f16_bits_to_f32_bits(s[0]));
            atomicAdd(&r->n_total, (unsigned long long)s[1]);
            if (s[2]) atomicAdd(&r->n_cross_clipped, (unsigned long long)s[2]);
            if (s[3]) atomicAdd(&r->n_clamped, (unsigned long long)s[3]);
            if (s[4]) atomicAdd(&r->n_nonfinite, (unsigned long long)s[4]);
        }
    }
}

}  // namespace

hipError_t launch_range_scan(const RangeScanItem* table_dev, int n_items, RangeScanRecord* rec_dev, int max_rows,
                             hipStream_t s) {
    if (n_items <= 0) return hipSuccess;
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return hipErrorInvalidDevice;
        cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    // persistent grid: four workgroups of four waves per CU (the kernel needs few registers), never more than there are rows
    int grid = cus * 4;
    if (grid > max_rows) grid = max_rows;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(range_scan_kernel, dim3(grid), dim3(kThreads), 0, s, table_dev, n_items, rec_dev);
    return hipGetLastError();
}

}  // namespace msr

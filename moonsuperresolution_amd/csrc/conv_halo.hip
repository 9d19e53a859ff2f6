#include "conv_common.h"
#include "conv_epilogue.h"

namespace msr {

// ------------------------------------------------------------------------------------------------------
// conv_igemm_bf16x3_halo: split-bf16, 3x3 stride 1, LDS-staged INPUT HALO tile.
//
// The generic kernel re-stages the 128-pixel activation tile for each of the 9 taps.  Here the workgroup's
// 8 x 16 pixel tile is staged once per 32-channel chunk together with its one-pixel halo ((8+2) x (16+2) = 180
// pixels x 128 bytes) and the nine taps read it at nine constant LDS offsets: activation traffic (global -> LDS
// and LDS writes) drops ~9x; the weight tile (128 channels x 128 bytes per K-step) is double-buffered as before.
// K order: chunk outer, tap inner (unrolled).  At the chunk seam: barrier, halo write, barrier.
// LDS: 180*144 + 2*128*144 = 62.8 KB -> 2 workgroups per CU.
// ------------------------------------------------------------------------------------------------------
template <int EPI, int SH>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv_igemm_bf16x3_halo(const ConvParams p, const TileGeom g) {
    constexpr int WM = 2, WN = 2, MT = 2, NT = 2;
    constexpr int NTHR = 256, BM = 128, BN = 128, BKC = 32, BKP = SH ? 40 : 36;
    constexpr int TH = 8, TW = 16, HH = TH + 2, HW = TW + 2, HP = HH * HW;   // 180 halo pixels
    constexpr int H_ITEMS = (HP * 8 + NTHR - 1) / NTHR;                        // 6 16-byte items per thread
    static_assert(H_ITEMS == 6, "halo staging is written for 6 items per thread");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const Ah = smem;                       // [HP][BKP]
    float* const Bs = smem + HP * BKP;            // [2][BN][BKP]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;

    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tn = bid % g.tiles_n;
    int tmi = bid / g.tiles_n;
    const int tx0 = (tmi % g.tiles_x) << g.tw_l;
    tmi /= g.tiles_x;
    const int ty0 = (tmi % g.tiles_y) << g.th_l;
    const int b0 = tmi / g.tiles_y;               // tb == 1
    const int n0 = tn * BN;

    // halo staging items (items past the end duplicate the last one: same bytes to the same LDS slot)
    int h_goff[H_ITEMS], h_loff[H_ITEMS];
#pragma unroll
    for (int q = 0; q < H_ITEMS; ++q) {
        int idx = tid + q * NTHR;
        idx = idx < HP * 8 ? idx : HP * 8 - 1;
        const int hp = idx >> 3, seg = idx & 7;
        const int hy = hp / HW, hx = hp - hy * HW;
        h_goff[q] = b0 * p.in_pb + (ty0 + hy) * p.in_py + (tx0 + hx) * p.Cin + seg * 4;
        h_loff[q] = hp * BKP + seg * 4;
    }
    int b_goff[4], b_loff[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = tid + q * NTHR;
        const int row = idx >> 3, seg = idx & 7;
        b_goff[q] = (n0 + row) * p.Cin + seg * 4;
        b_loff[q] = row * BKP + seg * 4;
    }
    // SH == 1: v_mfma_f32_16x16x32_bf16, lane (i = lane & 15, g = lane >> 4) holds row i, k = 8g + {0..7}
    int a_frag16[4], b_frag16[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a_frag16[i] = ((wm * 4 + i) * HW + (lane & 15)) * BKP + 4 * (lane >> 4);
        b_frag16[i] = ((wn * 4 + i) * 16 + (lane & 15)) * BKP + 4 * (lane >> 4);
    }
    f32x4 acc16[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc16[i][j][r] = 0.f;
    int a_frag[MT], b_frag[NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int row = (wm * MT + m) * 32 + l31;          // pixel (row >> 4, row & 15) of the 8 x 16 tile
        a_frag[m] = ((row >> 4) * HW + (row & 15)) * BKP + 4 * half;
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) b_frag[n] = ((wn * NT + n) * 32 + l31) * BKP + 4 * half;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    const int chunks = p.Cin / BKC;               // even (Cin % 64 == 0): the loop body is a PAIR of chunks
    // Buffer loads: a wave-uniform descriptor + a constant per-lane byte offset (VGPR) + a scalar byte offset that
    // carries the K-step; no 64-bit per-lane address arithmetic in the unrolled loop.
    const unsigned w_tap_bytes = (unsigned)((size_t)p.N * p.Cin * sizeof(float));
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.in), 0, (int)((size_t)p.B * p.in_pb * sizeof(float)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_wt = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.wt), 0, (int)(9u * w_tap_bytes), 0x00020000);
    unsigned h_pair = 0;                          // byte offset of the current chunk pair in a pixel
    unsigned w_pair = 0;                          // byte offset of the current chunk pair in a weight row
#pragma unroll
    for (int q = 0; q < H_ITEMS; ++q) h_goff[q] *= 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) b_goff[q] *= 4;

    float4 rh0, rh1, rh2, rh3, rh4, rh5;
    float4 re0, re1, re2, re3;                    // weights of even K-steps in flight
    float4 ro0, ro1, ro2, ro3;                    // weights of odd K-steps in flight
#define MSR_BUFLD(rs, voff, soff) \
    __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, (int)(soff), 0))
#define MSR_LOAD_H(soff)                                                                         \
    {                                                                                            \
        rh0 = MSR_BUFLD(rs_in, h_goff[0], soff);                                                 \
        rh1 = MSR_BUFLD(rs_in, h_goff[1], soff);                                                 \
        rh2 = MSR_BUFLD(rs_in, h_goff[2], soff);                                                 \
        rh3 = MSR_BUFLD(rs_in, h_goff[3], soff);                                                 \
        rh4 = MSR_BUFLD(rs_in, h_goff[4], soff);                                                 \
        rh5 = MSR_BUFLD(rs_in, h_goff[5], soff);                                                 \
    }
#define MSR_WRITE_H()                                                                            \
    {                                                                                            \
        *reinterpret_cast<float4*>(Ah + h_loff[0]) = rh0;                                        \
        *reinterpret_cast<float4*>(Ah + h_loff[1]) = rh1;                                        \
        *reinterpret_cast<float4*>(Ah + h_loff[2]) = rh2;                                        \
        *reinterpret_cast<float4*>(Ah + h_loff[3]) = rh3;                                        \
        *reinterpret_cast<float4*>(Ah + h_loff[4]) = rh4;                                        \
        *reinterpret_cast<float4*>(Ah + h_loff[5]) = rh5;                                        \
    }
// weights of K-step U of the current pair (U = 18, 19 are the first two steps of the next pair)
#define MSR_WPTR(U) (w_pair + ((U) / 9) * (BKC * 4) + (unsigned)((U) % 9) * w_tap_bytes)
#define MSR_LOAD_B(R, soff)                                                                      \
    {                                                                                            \
        R##0 = MSR_BUFLD(rs_wt, b_goff[0], soff);                                                \
        R##1 = MSR_BUFLD(rs_wt, b_goff[1], soff);                                                \
        R##2 = MSR_BUFLD(rs_wt, b_goff[2], soff);                                                \
        R##3 = MSR_BUFLD(rs_wt, b_goff[3], soff);                                                \
    }
#define MSR_WRITE_B(buf, R)                                                                      \
    {                                                                                            \
        float* b_ = Bs + (buf) * BN * BKP;                                                       \
        *reinterpret_cast<float4*>(b_ + b_loff[0]) = R##0;                                       \
        *reinterpret_cast<float4*>(b_ + b_loff[1]) = R##1;                                       \
        *reinterpret_cast<float4*>(b_ + b_loff[2]) = R##2;                                       \
        *reinterpret_cast<float4*>(b_ + b_loff[3]) = R##3;                                       \
    }
#define MSR_COMPUTE(buf, TAP)                                                                    \
    {                                                                                            \
        const float* a_ = Ah + (((TAP) / 3) * HW + ((TAP) % 3)) * BKP;                           \
        const float* b_ = Bs + (buf) * BN * BKP;                                                 \
        if constexpr (SH == 1) {                                                                 \
            bf16x8 ah[4], al[4];                                                                 \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                      \
                ah[i] = *reinterpret_cast<const bf16x8*>(a_ + a_frag16[i]);                      \
                al[i] = *reinterpret_cast<const bf16x8*>(a_ + a_frag16[i] + 16);                 \
            }                                                                                    \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                      \
                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(b_ + b_frag16[j]);            \
                const bf16x8 bl = *reinterpret_cast<const bf16x8*>(b_ + b_frag16[j] + 16);       \
                _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                  \
                    /* weights as the row operand: D[channel][pixel], see halo16_epilogue_body */ \
                    acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, al[i], acc16[i][j], 0, 0, 0); \
                    acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl, ah[i], acc16[i][j], 0, 0, 0); \
                    acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ah[i], acc16[i][j], 0, 0, 0); \
                }                                                                                \
            }                                                                                    \
        } else                                                                                   \
        _Pragma("unroll") for (int kg = 0; kg < 2; ++kg) {                                       \
            bf16x8 ah[MT], al[MT], bh[NT], bl[NT];                                               \
            _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                     \
                ah[m] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[m] + kg * 8);               \
                al[m] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[m] + kg * 8 + 16);          \
            }                                                                                    \
            _Pragma("unroll") for (int n = 0; n < NT; ++n) {                                     \
                bh[n] = *reinterpret_cast<const bf16x8*>(b_ + b_frag[n] + kg * 8);               \
                bl[n] = *reinterpret_cast<const bf16x8*>(b_ + b_frag[n] + kg * 8 + 16);          \
            }                                                                                    \
            _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                     \
                _Pragma("unroll") for (int n = 0; n < NT; ++n) {                                 \
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[m], bh[n], acc[m][n], 0, 0, 0); \
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[m], bl[n], acc[m][n], 0, 0, 0); \
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[m], bh[n], acc[m][n], 0, 0, 0); \
                }                                                                                \
            }                                                                                    \
        }                                                                                        \
    }
// K-step T (0..17, compile time) of a chunk pair.  Weights of step T+2 are requested into LD (the set that step
// T's weights have just left), the MFMAs of step T run from LDS buffer T & 1, then the weights of step T+1 (set
// WR, requested one step ago) go to the other buffer.  The halo of the next chunk is requested on tap 7 and
// replaces the old one after tap 8.  LASTP (compile time) drops everything that would reach past the last pair,
// so no load or LDS write sits under a run-time condition (hipcc would wait vmcnt(0) around those).
#define MSR_STEP(T, LD, WR, LASTP)                                                               \
    {                                                                                            \
        if (!(LASTP) || (T) + 2 < 18) MSR_LOAD_B(LD, MSR_WPTR((T) + 2));                         \
        if ((T) == 7) MSR_LOAD_H(h_pair + BKC * 4);                                              \
        if ((T) == 16 && !(LASTP)) MSR_LOAD_H(h_pair + 2 * BKC * 4);                             \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        MSR_COMPUTE((T) & 1, (T) % 9);                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        if (!(LASTP) || (T) + 1 < 18) MSR_WRITE_B(((T) & 1) ^ 1, WR);                            \
        if ((T) == 8 || ((T) == 17 && !(LASTP))) {                                               \
            __syncthreads();            /* every wave is done with the old halo */               \
            MSR_WRITE_H();                                                                       \
        }                                                                                        \
        if (!(LASTP) || (T) + 1 < 18) __syncthreads();                                           \
    }
#define MSR_PAIR(LASTP)                                                                          \
    MSR_STEP(0, re, ro, LASTP) MSR_STEP(1, ro, re, LASTP) MSR_STEP(2, re, ro, LASTP)             \
    MSR_STEP(3, ro, re, LASTP) MSR_STEP(4, re, ro, LASTP) MSR_STEP(5, ro, re, LASTP)             \
    MSR_STEP(6, re, ro, LASTP) MSR_STEP(7, ro, re, LASTP) MSR_STEP(8, re, ro, LASTP)             \
    MSR_STEP(9, ro, re, LASTP) MSR_STEP(10, re, ro, LASTP) MSR_STEP(11, ro, re, LASTP)           \
    MSR_STEP(12, re, ro, LASTP) MSR_STEP(13, ro, re, LASTP) MSR_STEP(14, re, ro, LASTP)          \
    MSR_STEP(15, ro, re, LASTP) MSR_STEP(16, re, ro, LASTP) MSR_STEP(17, ro, re, LASTP)

    // prologue: halo of chunk 0 and the weights of step 0 into LDS, the weights of step 1 stay in flight
    MSR_LOAD_H(h_pair);
    MSR_LOAD_B(re, MSR_WPTR(0));
    MSR_LOAD_B(ro, MSR_WPTR(1));
    MSR_WRITE_H();
    MSR_WRITE_B(0, re);
    __syncthreads();
    for (int pr = 0; pr < chunks / 2 - 1; ++pr) {
        MSR_PAIR(false)
        h_pair += 2 * BKC * 4;
        w_pair += 2 * BKC * 4;
    }
    MSR_PAIR(true)
#undef MSR_BUFLD
#undef MSR_LOAD_H
#undef MSR_WRITE_H
#undef MSR_WPTR
#undef MSR_LOAD_B
#undef MSR_WRITE_B
#undef MSR_COMPUTE
#undef MSR_STEP
#undef MSR_PAIR

    if constexpr (SH == 1) {
        float4 xin[4][2], cv[8];
        halo16_epilogue_load<EPI>(p, xin, cv, wm, wn, lane, n0, tx0, ty0, b0);
        halo16_epilogue<EPI>(p, g, acc16, wm, wn, lane, n0, tx0, ty0, b0, xin, cv);
    }
    else conv_epilogue<WM, WN, MT, NT, EPI>(p, g, acc, 0, wm, wn, half, l31, n0, tx0, ty0, b0);
}

static constexpr size_t HALO_LDS = (size_t)(180 + 2 * 128) * 36 * sizeof(float);
static constexpr size_t HALO16_LDS = (size_t)(180 + 2 * 128) * 40 * sizeof(float);

hipError_t set_attr_halo() {
    hipError_t e;
#define MSR_SET(EPI)                                                                                          \
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm_bf16x3_halo<EPI, 0>),               \
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)HALO_LDS)) != hipSuccess)    \
        return e;                                                                                             \
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm_bf16x3_halo<EPI, 1>),               \
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)HALO16_LDS)) != hipSuccess)  \
        return e;
    MSR_SET(EPI_BIAS) MSR_SET(EPI_RES) MSR_SET(EPI_SPADE)
#undef MSR_SET
    return hipSuccess;
}

hipError_t launch_halo(const ConvParams& p, int epi, int sh, hipStream_t s) {
    TileGeom g;
    if (!make_geom(p, 128, 128, 32, g)) return hipErrorInvalidValue;
    if (g.tb != 1 || g.th_l != 3 || g.tw_l != 4 || p.stride != 1 || p.KH != 3 || p.KW != 3 || p.ksplit > 1 ||
        p.Cin % 64)   // the K loop is unrolled by two steps: 9 * (Cin / 32) must be even
        return hipErrorInvalidValue;
    if ((size_t)p.B * p.in_pb * sizeof(float) >= ((size_t)1 << 31)) return hipErrorInvalidValue;   // buffer descriptor range
    if (sh) {
        switch (epi) {
            case EPI_BIAS: conv_igemm_bf16x3_halo<EPI_BIAS, 1><<<g.tiles_mn, 256, HALO16_LDS, s>>>(p, g); break;
            case EPI_RES: conv_igemm_bf16x3_halo<EPI_RES, 1><<<g.tiles_mn, 256, HALO16_LDS, s>>>(p, g); break;
            case EPI_SPADE: conv_igemm_bf16x3_halo<EPI_SPADE, 1><<<g.tiles_mn, 256, HALO16_LDS, s>>>(p, g); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (epi) {
        case EPI_BIAS: conv_igemm_bf16x3_halo<EPI_BIAS, 0><<<g.tiles_mn, 256, HALO_LDS, s>>>(p, g); break;
        case EPI_RES: conv_igemm_bf16x3_halo<EPI_RES, 0><<<g.tiles_mn, 256, HALO_LDS, s>>>(p, g); break;
        case EPI_SPADE: conv_igemm_bf16x3_halo<EPI_SPADE, 0><<<g.tiles_mn, 256, HALO_LDS, s>>>(p, g); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace msr

// conv_igemm — NHWC implicit-GEMM convolution for gfx950: exact fp32 on v_mfma_f32_32x32x2_f32, or 3-term
// split-bf16 ("bf16x3") on v_mfma_f32_32x32x16_bf16 (see kernels.h ConvPrecision).
//
// Replaces the cuDNN/Eigen Conv2D calls behind spade.py:10-11,19-20 (gamma/beta convs, 49.9 % of the
// generator's FLOPs) and blocks.py:19-20,26,30-34 (ResidualBlock convs, 48.5 %), plus the strided
// encoder convs of blocks.py:52-61.  fp32-in / fp32-accumulate MFMA is bit-for-bit an fmaf chain
// (MI355X_MICROARCH.md "Matrix cores"), so parity with the fp32 reference holds at fp32 rounding.
//
// Structure (per workgroup of WM x WN waves):
//   tile  BM = WM*MT*32 output pixels  x  BN = WN*NT*32 output channels, K-step = 32 channels of one tap
//   A (pixels x k) and B (channels x k) tiles are staged global -> VGPR -> LDS with 16-byte accesses,
//   double-buffered, one barrier per K-step, loads for step t+1 issued before the MFMAs of step t.
//   LDS rows are [row][32 k + 4 pad] floats: the 144-byte pitch makes the ds_read_b128 fragment reads
//   bank-conflict free (16 lanes of a read group hit 16 distinct 16-byte slots).
//   Fragment trick: lane (i, h) reads k = 8*kk + 4*h + {0..3} as ONE ds_read_b128 and feeds element s
//   to MFMA s; the B lane reads the same k, so the four MFMAs cover the 8 k's exactly once.
//   Each wave owns MT x NT accumulator tiles of 32x32 (64 VGPRs for 2x2).
//   The input tensor carries a physical zero border, so no bounds checks exist in the K loop.
#include "conv_common.h"
#include "conv_epilogue.h"

namespace msr {

// K-step = BKC channels of one tap; LDS rows are BKC + 4 floats.  Both pitches (36 and 20 floats) put the 16
// lanes of a ds_read_b128 group on 16 distinct 16-byte slots, i.e. the fragment reads are conflict-free.
//
// LDS staging store of one 16-byte global item: a plain copy for both precisions (split-bf16 tensors already hold
// the [32 hi | 32 lo] chunk image in HBM, see kernels.h).
template <int PREC>
__device__ __forceinline__ void stage_store(float* dst, const float4& v) {
    *reinterpret_cast<float4*>(dst) = v;
}

template <int WM, int WN, int MT, int NT, int BKC, int EPI, int PREC>
__global__ void __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(2, BKC == 16 ? 3 : 2)))
conv_igemm(const ConvParams p, const TileGeom g) {
    static_assert(PREC == PREC_F32 || BKC == 32, "the split-bf16 path uses the 32-channel K-step");
    constexpr int NTHR = WM * WN * 64;
    constexpr int BM = WM * MT * 32;
    constexpr int BN = WN * NT * 32;
    constexpr int BKP = BKC + 4;
    constexpr int SEGS = BKC / 4;            // 16-byte segments per staged row
    constexpr int A_ITEMS = BM * SEGS / NTHR;
    constexpr int B_ITEMS = BN * SEGS / NTHR;
    static_assert(BM * SEGS % NTHR == 0 && BN * SEGS % NTHR == 0, "staging split");
    static_assert(EPI != EPI_SPADE || NT % 2 == 0, "SPADE epilogue pairs gamma/beta sub-tiles");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;                      // [2][BM][BKP]
    float* const Bs = smem + 2 * BM * BKP;       // [2][BN][BKP]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;

    const int bid_all = xcd_remap(blockIdx.x, gridDim.x);
    const int ks = bid_all / g.tiles_mn;          // split-K range index (0 when ksplit == 1)
    const int bid = bid_all - ks * g.tiles_mn;
    const int tn = bid % g.tiles_n;
    int tmi = bid / g.tiles_n;
    const int tx0 = (tmi % g.tiles_x) << g.tw_l;
    tmi /= g.tiles_x;
    const int ty0 = (tmi % g.tiles_y) << g.th_l;
    const int b0 = (tmi / g.tiles_y) * g.tb;
    const int n0 = tn * BN;
    const int twm = (1 << g.tw_l) - 1, thm = (1 << g.th_l) - 1;

    // ---- staging assignments ------------------------------------------------------------------
    int a_goff[A_ITEMS];   // global float offset of this thread's A rows (tap (0,0), channel chunk 0)
    int a_loff[A_ITEMS];
#pragma unroll
    for (int q = 0; q < A_ITEMS; ++q) {
        const int idx = tid + q * NTHR;
        const int row = idx / SEGS, seg = idx % SEGS;
        const int tx = row & twm, ty = (row >> g.tw_l) & thm, tbi = row >> (g.tw_l + g.th_l);
        int b = b0 + tbi;
        b = b < p.B ? b : p.B - 1;   // rows past the batch read valid memory and are dropped in the epilogue
        a_goff[q] = b * p.in_pb + (ty0 + ty) * p.stride * p.in_py + (tx0 + tx) * p.stride * p.in_px + seg * 4;
        a_loff[q] = row * BKP + seg * 4;
    }
    int b_goff[B_ITEMS];
    int b_loff[B_ITEMS];
#pragma unroll
    for (int q = 0; q < B_ITEMS; ++q) {
        const int idx = tid + q * NTHR;
        const int row = idx / SEGS, seg = idx % SEGS;
        b_goff[q] = (n0 + row) * p.Cin + seg * 4;
        b_loff[q] = row * BKP + seg * 4;
    }

    // ---- fragment read offsets ------------------------------------------------------------------
    int a_frag[MT], b_frag[NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) a_frag[m] = ((wm * MT + m) * 32 + l31) * BKP + 4 * half;
#pragma unroll
    for (int n = 0; n < NT; ++n) b_frag[n] = ((wn * NT + n) * 32 + l31) * BKP + 4 * half;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    const int taps = p.KH * p.KW;
    const int chunks = p.Cin / BKC;
    const int steps = taps * chunks;
    const size_t w_tap_stride = (size_t)p.N * p.Cin;

    // K-step iterator, kept as running scalars (no divisions in the loop).  With split-K this workgroup owns steps
    // [t_begin, t_end).  Order: BKC = 32 -> channel chunk outer, tap inner; BKC = 16 -> tap outer, chunk inner, so
    // that consecutive steps read the two 64-byte halves of the same 128-byte lines.
    const int t_begin = (int)((long)ks * steps / p.ksplit), t_end = (int)((long)(ks + 1) * steps / p.ksplit);
    int it_kh, it_kw, it_cc;
    const float* a_src;
    const float* b_src;
    if constexpr (BKC == 32) {
        const int cc0 = t_begin / taps, tap0 = t_begin - cc0 * taps;
        it_cc = cc0; it_kh = tap0 / p.KW; it_kw = tap0 - it_kh * p.KW;
        a_src = p.in + (it_kh * p.in_py + it_kw * p.in_px + cc0 * BKC);
        b_src = p.wt + ((size_t)tap0 * w_tap_stride + cc0 * BKC);
    } else {
        const int tap0 = t_begin / chunks, cc0 = t_begin - tap0 * chunks;
        it_cc = cc0; it_kh = tap0 / p.KW; it_kw = tap0 - it_kh * p.KW;
        a_src = p.in + (it_kh * p.in_py + it_kw * p.in_px + cc0 * BKC);
        b_src = p.wt + ((size_t)tap0 * w_tap_stride + cc0 * BKC);
    }

    // Named scalars, not arrays: hipcc leaves a float4 array that crosses a sched_barrier in scratch memory.
    static_assert((A_ITEMS == 4 || A_ITEMS == 2) && A_ITEMS == B_ITEMS, "staging is written for 2+2 or 4+4 items");
    float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
#define MSR_ISSUE_LOADS()                                                                        \
    {                                                                                            \
        ra0 = *reinterpret_cast<const float4*>(a_src + a_goff[0]);                               \
        ra1 = *reinterpret_cast<const float4*>(a_src + a_goff[1]);                               \
        if constexpr (A_ITEMS == 4) {                                                            \
            ra2 = *reinterpret_cast<const float4*>(a_src + a_goff[2]);                           \
            ra3 = *reinterpret_cast<const float4*>(a_src + a_goff[3]);                           \
        }                                                                                        \
        rb0 = *reinterpret_cast<const float4*>(b_src + b_goff[0]);                               \
        rb1 = *reinterpret_cast<const float4*>(b_src + b_goff[1]);                               \
        if constexpr (B_ITEMS == 4) {                                                            \
            rb2 = *reinterpret_cast<const float4*>(b_src + b_goff[2]);                           \
            rb3 = *reinterpret_cast<const float4*>(b_src + b_goff[3]);                           \
        }                                                                                        \
    }
#define MSR_ADVANCE()                                                                            \
    {                                                                                            \
        if constexpr (BKC == 32) {                                                               \
            ++it_kw;                                                                             \
            a_src += p.in_px;                                                                    \
            b_src += w_tap_stride;                                                               \
            if (it_kw == p.KW) {                                                                 \
                it_kw = 0;                                                                       \
                ++it_kh;                                                                         \
                a_src += p.in_py - p.KW * p.in_px;                                               \
                if (it_kh == p.KH) {                                                             \
                    it_kh = 0;                                                                   \
                    a_src += BKC - p.KH * p.in_py;                                               \
                    b_src += BKC - (size_t)taps * w_tap_stride;                                  \
                }                                                                                \
            }                                                                                    \
        } else {                                                                                 \
            ++it_cc;                                                                             \
            a_src += BKC;                                                                        \
            b_src += BKC;                                                                        \
            if (it_cc == chunks) {                                                               \
                it_cc = 0;                                                                       \
                ++it_kw;                                                                         \
                a_src += p.in_px - chunks * BKC;                                                 \
                b_src += w_tap_stride - chunks * BKC;                                            \
                if (it_kw == p.KW) {                                                             \
                    it_kw = 0;                                                                   \
                    ++it_kh;                                                                     \
                    a_src += p.in_py - p.KW * p.in_px;                                           \
                }                                                                                \
            }                                                                                    \
        }                                                                                        \
    }
#define MSR_WRITE_LDS(buf)                                                                       \
    {                                                                                            \
        float* a_ = As + (buf) * BM * BKP;                                                       \
        float* b_ = Bs + (buf) * BN * BKP;                                                       \
        stage_store<PREC>(a_ + a_loff[0], ra0);                                                  \
        stage_store<PREC>(a_ + a_loff[1], ra1);                                                  \
        if constexpr (A_ITEMS == 4) {                                                            \
            stage_store<PREC>(a_ + a_loff[2], ra2);                                              \
            stage_store<PREC>(a_ + a_loff[3], ra3);                                              \
        }                                                                                        \
        stage_store<PREC>(b_ + b_loff[0], rb0);                                                  \
        stage_store<PREC>(b_ + b_loff[1], rb1);                                                  \
        if constexpr (B_ITEMS == 4) {                                                            \
            stage_store<PREC>(b_ + b_loff[2], rb2);                                              \
            stage_store<PREC>(b_ + b_loff[3], rb3);                                              \
        }                                                                                        \
    }
#define MSR_COMPUTE(buf)                                                                         \
    {                                                                                            \
        const float* a_ = As + (buf) * BM * BKP;                                                 \
        const float* b_ = Bs + (buf) * BN * BKP;                                                 \
        if constexpr (PREC == PREC_F32) {                                                        \
            _Pragma("unroll") for (int kk = 0; kk < BKC / 8; ++kk) {                             \
                float4 fa[MT], fb[NT];                                                           \
                _Pragma("unroll") for (int m = 0; m < MT; ++m)                                   \
                    fa[m] = *reinterpret_cast<const float4*>(a_ + a_frag[m] + kk * 8);           \
                _Pragma("unroll") for (int n = 0; n < NT; ++n)                                   \
                    fb[n] = *reinterpret_cast<const float4*>(b_ + b_frag[n] + kk * 8);           \
                _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                  \
                    _Pragma("unroll") for (int m = 0; m < MT; ++m) {                             \
                        const float av = s == 0 ? fa[m].x : s == 1 ? fa[m].y : s == 2 ? fa[m].z : fa[m].w; \
                        _Pragma("unroll") for (int n = 0; n < NT; ++n) {                         \
                            const float bv = s == 0 ? fb[n].x : s == 1 ? fb[n].y : s == 2 ? fb[n].z : fb[n].w; \
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[m][n], 0, 0, 0); \
                        }                                                                        \
                    }                                                                            \
                }                                                                                \
            }                                                                                    \
        } else {                                                                                 \
            /* rows are [32 hi bf16 | 32 lo bf16 | pad]; lane (i, h) takes k = 16*kg + 8*h + {0..7} */ \
            _Pragma("unroll") for (int kg = 0; kg < 2; ++kg) {                                   \
                bf16x8 ah[MT], al[MT], bh[NT], bl[NT];                                           \
                _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                 \
                    ah[m] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[m] + kg * 8);           \
                    al[m] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[m] + kg * 8 + 16);      \
                }                                                                                \
                _Pragma("unroll") for (int n = 0; n < NT; ++n) {                                 \
                    bh[n] = *reinterpret_cast<const bf16x8*>(b_ + b_frag[n] + kg * 8);           \
                    bl[n] = *reinterpret_cast<const bf16x8*>(b_ + b_frag[n] + kg * 8 + 16);      \
                }                                                                                \
                _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                 \
                    _Pragma("unroll") for (int n = 0; n < NT; ++n) {                             \
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[m], bh[n], acc[m][n], 0, 0, 0); \
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[m], bl[n], acc[m][n], 0, 0, 0); \
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[m], bh[n], acc[m][n], 0, 0, 0); \
                    }                                                                            \
                }                                                                                \
            }                                                                                    \
        }                                                                                        \
    }

    MSR_ISSUE_LOADS();
    MSR_WRITE_LDS(0);
    __syncthreads();
    int cur = 0;
    for (int t = t_begin; t < t_end - 1; ++t) {
        MSR_ADVANCE();
        MSR_ISSUE_LOADS();       // global loads of step t+1 fly while the MFMAs of step t run
        __builtin_amdgcn_sched_barrier(0);   // keep hipcc from sinking the loads below the MFMAs
        MSR_COMPUTE(cur);
        __builtin_amdgcn_sched_barrier(0);
        MSR_WRITE_LDS(cur ^ 1);  // the other buffer was last read before the previous barrier
        __syncthreads();
        cur ^= 1;
    }
    MSR_COMPUTE(cur);
#undef MSR_ISSUE_LOADS
#undef MSR_ADVANCE
#undef MSR_WRITE_LDS
#undef MSR_COMPUTE

    // the 16-channel K-step variant must stay under 168 VGPRs (3 workgroups per CU): small load batches there
    conv_epilogue<WM, WN, MT, NT, EPI, (BKC == 16 ? 4 : 16)>(p, g, acc, ks, wm, wn, half, l31, n0, tx0, ty0, b0);
}

// ------------------------------------------------------------------------------------------------------
template <int WM, int WN, int MT, int NT, int BKC>
struct TileCfg {
    static constexpr int BM = WM * MT * 32, BN = WN * NT * 32, NTHR = WM * WN * 64;
    static constexpr size_t LDS = (size_t)(2 * BM + 2 * BN) * (BKC + 4) * sizeof(float);
};
// TILE_128x128   : 4 waves, K-step 32, 72 KiB LDS -> 2 workgroups (2 waves / SIMD) per CU
// TILE_64x64     : 2 waves, K-step 32, 36 KiB LDS -> 4 workgroups per CU (low-resolution layers, with split-K)
// TILE_128x128_K16: 4 waves, K-step 16, 40 KiB LDS -> 3 workgroups (3 waves / SIMD) per CU

template <int WM, int WN, int MT, int NT, int BKC, int EPI, int PREC>
static hipError_t set_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm<WM, WN, MT, NT, BKC, EPI, PREC>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)TileCfg<WM, WN, MT, NT, BKC>::LDS);
}

template <int WM, int WN, int MT, int NT, int BKC, int PREC>
static hipError_t set_attr_all() {
    hipError_t e;
    if ((e = set_attr<WM, WN, MT, NT, BKC, EPI_BIAS, PREC>()) != hipSuccess) return e;
    if ((e = set_attr<WM, WN, MT, NT, BKC, EPI_RES, PREC>()) != hipSuccess) return e;
    if ((e = set_attr<WM, WN, MT, NT, BKC, EPI_SPADE, PREC>()) != hipSuccess) return e;
    if ((e = set_attr<WM, WN, MT, NT, BKC, EPI_AFFINE, PREC>()) != hipSuccess) return e;
    return set_attr<WM, WN, MT, NT, BKC, EPI_PARTIAL, PREC>();
}

hipError_t set_attr_generic() {
    hipError_t e;
    if ((e = set_attr_all<2, 2, 2, 2, 32, PREC_F32>()) != hipSuccess) return e;
    if ((e = set_attr_all<2, 1, 1, 2, 32, PREC_F32>()) != hipSuccess) return e;
    if ((e = set_attr_all<2, 2, 2, 2, 16, PREC_F32>()) != hipSuccess) return e;
    if ((e = set_attr_all<2, 2, 2, 2, 32, PREC_BF16X3>()) != hipSuccess) return e;
    return set_attr_all<2, 1, 1, 2, 32, PREC_BF16X3>();
}

template <int WM, int WN, int MT, int NT, int BKC, int PREC>
static hipError_t launch_cfg(const ConvParams& p, int epi, hipStream_t s) {
    using C = TileCfg<WM, WN, MT, NT, BKC>;
    TileGeom g;
    if (!make_geom(p, C::BM, C::BN, BKC, g)) return hipErrorInvalidValue;
    if (p.ksplit > 1) {
        if (!p.partial || (epi != EPI_BIAS && epi != EPI_RES && epi != EPI_SPADE && epi != EPI_AFFINE)) return hipErrorInvalidValue;
        conv_igemm<WM, WN, MT, NT, BKC, EPI_PARTIAL, PREC><<<g.tiles_mn * p.ksplit, C::NTHR, C::LDS, s>>>(p, g);
        return finish_splitk(p, epi, s);
    }
    const int grid = g.tiles_mn;
    switch (epi) {
        case EPI_AFFINE:
            conv_igemm<WM, WN, MT, NT, BKC, EPI_AFFINE, PREC><<<grid, C::NTHR, C::LDS, s>>>(p, g);
            break;
        case EPI_BIAS:
            conv_igemm<WM, WN, MT, NT, BKC, EPI_BIAS, PREC><<<grid, C::NTHR, C::LDS, s>>>(p, g);
            break;
        case EPI_RES:
            conv_igemm<WM, WN, MT, NT, BKC, EPI_RES, PREC><<<grid, C::NTHR, C::LDS, s>>>(p, g);
            break;
        case EPI_SPADE:
            conv_igemm<WM, WN, MT, NT, BKC, EPI_SPADE, PREC><<<grid, C::NTHR, C::LDS, s>>>(p, g);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_generic(const ConvParams& p, int epi, int tile, hipStream_t s) {
    if (p.prec == PREC_BF16X3) {
        if (tile == TILE_64x64) return launch_cfg<2, 1, 1, 2, 32, PREC_BF16X3>(p, epi, s);
        return launch_cfg<2, 2, 2, 2, 32, PREC_BF16X3>(p, epi, s);
    }
    if (tile == TILE_128x128) return launch_cfg<2, 2, 2, 2, 32, PREC_F32>(p, epi, s);
    if (tile == TILE_128x128_K16) return launch_cfg<2, 2, 2, 2, 16, PREC_F32>(p, epi, s);
    return launch_cfg<2, 1, 1, 2, 32, PREC_F32>(p, epi, s);
}

}  // namespace msr

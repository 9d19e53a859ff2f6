#include "conv_common.h"
#include "conv_epilogue.h"

namespace msr {

// ------------------------------------------------------------------------------------------------------
// conv_igemm_bf16x3: the split-bf16 kernel with the WEIGHT operand kept out of LDS.
//
// At bf16 MFMA rates the 128x128 tile is LDS-bound (staging writes + fragment reads of both operands use ~85 % of
// the LDS), so the weights are stored in HBM in MFMA-fragment order,
//     wt[tap][chunk][n-tile of 32][kg][hi|lo][lane 0..63][8 bf16]          (1 KiB per wave-instruction)
// and every wave loads its own B fragments straight into VGPRs with coalesced global_load_dwordx4, one K-step
// ahead (two named register sets, the loop is unrolled by two).  Only the activation tile goes through LDS
// (global -> VGPR -> LDS, double-buffered, one barrier per K-step, as in the fp32 kernel).
// ------------------------------------------------------------------------------------------------------
template <int WM, int WN, int MT, int NT, int EPI>
__global__ void __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv_igemm_bf16x3(const ConvParams p, const TileGeom g) {
    static_assert(NT == 2, "B register sets are written for two n-tiles per wave");
    constexpr int NTHR = WM * WN * 64;
    constexpr int BM = WM * MT * 32;
    constexpr int BN = WN * NT * 32;
    constexpr int BKC = 32, BKP = 36, SEGS = 8;
    constexpr int A_ITEMS = BM * SEGS / NTHR;
    static_assert(A_ITEMS == 4, "staging is written for 4 16-byte items per thread");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;                      // [2][BM][BKP]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;

    const int bid_all = xcd_remap(blockIdx.x, gridDim.x);
    const int ks = bid_all / g.tiles_mn;
    const int bid = bid_all - ks * g.tiles_mn;
    const int tn = bid % g.tiles_n;
    int tmi = bid / g.tiles_n;
    const int tx0 = (tmi % g.tiles_x) << g.tw_l;
    tmi /= g.tiles_x;
    const int ty0 = (tmi % g.tiles_y) << g.th_l;
    const int b0 = (tmi / g.tiles_y) * g.tb;
    const int n0 = tn * BN;
    const int twm = (1 << g.tw_l) - 1, thm = (1 << g.th_l) - 1;

    int a_goff[A_ITEMS], a_loff[A_ITEMS];
#pragma unroll
    for (int q = 0; q < A_ITEMS; ++q) {
        const int idx = tid + q * NTHR;
        const int row = idx / SEGS, seg = idx % SEGS;
        const int tx = row & twm, ty = (row >> g.tw_l) & thm, tbi = row >> (g.tw_l + g.th_l);
        int b = b0 + tbi;
        b = b < p.B ? b : p.B - 1;
        a_goff[q] = b * p.in_pb + (ty0 + ty) * p.stride * p.in_py + (tx0 + tx) * p.stride * p.Cin + seg * 4;
        a_loff[q] = row * BKP + seg * 4;
    }
    int a_frag[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) a_frag[m] = ((wm * MT + m) * 32 + l31) * BKP + 4 * half;

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
    const int nt32 = p.N / 32;
    // fragment-order weights: 1024 floats per (tap, chunk, n-tile): [kg][hi|lo][lane][4 floats]
    const size_t w_chunk_stride = (size_t)nt32 * 1024;           // next channel chunk, same tap
    const size_t w_tap_stride = (size_t)chunks * w_chunk_stride;  // next tap, same chunk

    const int t_begin = (int)((long)ks * steps / p.ksplit), t_end = (int)((long)(ks + 1) * steps / p.ksplit);
    const int cc0 = t_begin / taps, tap0 = t_begin - cc0 * taps;
    int it_kh = tap0 / p.KW, it_kw = tap0 - it_kh * p.KW;
    const float* a_src = p.in + (it_kh * p.in_py + it_kw * p.Cin + cc0 * BKC);
    const float* b_src = p.wt + (size_t)tap0 * w_tap_stride + (size_t)cc0 * w_chunk_stride +
                         (size_t)(n0 / 32 + wn * NT) * 1024 + lane * 4;

    float4 ra0, ra1, ra2, ra3;
    // B fragments of one K-step: [n-tile 0/1][kg 0/1][hi/lo]; two sets P (even steps) and Q (odd steps)
    bf16x8 P00h, P00l, P01h, P01l, P10h, P10l, P11h, P11l;
    bf16x8 Q00h, Q00l, Q01h, Q01l, Q10h, Q10l, Q11h, Q11l;

#define MSR_LDB(ptr, off) (*reinterpret_cast<const bf16x8*>((ptr) + (off)))
#define MSR_LOAD_B(S)                                                                            \
    {                                                                                            \
        S##00h = MSR_LDB(b_src, 0);        S##00l = MSR_LDB(b_src, 256);                         \
        S##01h = MSR_LDB(b_src, 512);      S##01l = MSR_LDB(b_src, 768);                         \
        S##10h = MSR_LDB(b_src, 1024);     S##10l = MSR_LDB(b_src, 1280);                        \
        S##11h = MSR_LDB(b_src, 1536);     S##11l = MSR_LDB(b_src, 1792);                        \
    }
#define MSR_LOAD_A()                                                                             \
    {                                                                                            \
        ra0 = *reinterpret_cast<const float4*>(a_src + a_goff[0]);                               \
        ra1 = *reinterpret_cast<const float4*>(a_src + a_goff[1]);                               \
        ra2 = *reinterpret_cast<const float4*>(a_src + a_goff[2]);                               \
        ra3 = *reinterpret_cast<const float4*>(a_src + a_goff[3]);                               \
    }
#define MSR_ADVANCE()                                                                            \
    {                                                                                            \
        ++it_kw;                                                                                 \
        a_src += p.Cin;                                                                          \
        b_src += w_tap_stride;                                                                   \
        if (it_kw == p.KW) {                                                                     \
            it_kw = 0;                                                                           \
            ++it_kh;                                                                             \
            a_src += p.in_py - p.KW * p.Cin;                                                     \
            if (it_kh == p.KH) {                                                                 \
                it_kh = 0;                                                                       \
                a_src += BKC - p.KH * p.in_py;                                                   \
                b_src += w_chunk_stride - (size_t)taps * w_tap_stride;                           \
            }                                                                                    \
        }                                                                                        \
    }
#define MSR_WRITE_A(buf)                                                                         \
    {                                                                                            \
        float* a_ = As + (buf) * BM * BKP;                                                       \
        *reinterpret_cast<float4*>(a_ + a_loff[0]) = ra0;                                        \
        *reinterpret_cast<float4*>(a_ + a_loff[1]) = ra1;                                        \
        *reinterpret_cast<float4*>(a_ + a_loff[2]) = ra2;                                        \
        *reinterpret_cast<float4*>(a_ + a_loff[3]) = ra3;                                        \
    }
#define MSR_MMA3(m, n, AH, AL, BH, BL)                                                           \
    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AL, BH, acc[m][n], 0, 0, 0);             \
    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH, BL, acc[m][n], 0, 0, 0);             \
    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH, BH, acc[m][n], 0, 0, 0);
#define MSR_COMPUTE(buf, S)                                                                      \
    {                                                                                            \
        const float* a_ = As + (buf) * BM * BKP;                                                 \
        bf16x8 ah[MT], al[MT];                                                                   \
        _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                         \
            ah[m] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[m]);                            \
            al[m] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[m] + 16);                       \
        }                                                                                        \
        _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                         \
            MSR_MMA3(m, 0, ah[m], al[m], S##00h, S##00l)                                         \
            MSR_MMA3(m, 1, ah[m], al[m], S##10h, S##10l)                                         \
        }                                                                                        \
        _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                         \
            ah[m] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[m] + 8);                        \
            al[m] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[m] + 8 + 16);                   \
        }                                                                                        \
        _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                         \
            MSR_MMA3(m, 0, ah[m], al[m], S##01h, S##01l)                                         \
            MSR_MMA3(m, 1, ah[m], al[m], S##11h, S##11l)                                         \
        }                                                                                        \
    }
#define MSR_STEP(CUR, NXT)                                                                       \
    {                                                                                            \
        MSR_ADVANCE();                                                                           \
        MSR_LOAD_A();                                                                            \
        MSR_LOAD_B(NXT);                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        MSR_COMPUTE(cur, CUR);                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        MSR_WRITE_A(cur ^ 1);                                                                    \
        __syncthreads();                                                                         \
        cur ^= 1;                                                                                \
    }

    MSR_LOAD_A();
    MSR_LOAD_B(P);
    MSR_WRITE_A(0);
    __syncthreads();
    int cur = 0;
    const int nsteps = t_end - t_begin;
    int i = 0;
    for (; i + 2 <= nsteps - 1; i += 2) {
        MSR_STEP(P, Q);
        MSR_STEP(Q, P);
    }
    if ((nsteps - 1) & 1) {
        MSR_STEP(P, Q);
        MSR_COMPUTE(cur, Q);
    } else {
        MSR_COMPUTE(cur, P);
    }
#undef MSR_LDB
#undef MSR_LOAD_B
#undef MSR_LOAD_A
#undef MSR_ADVANCE
#undef MSR_WRITE_A
#undef MSR_MMA3
#undef MSR_COMPUTE
#undef MSR_STEP

    conv_epilogue<WM, WN, MT, NT, EPI>(p, g, acc, ks, wm, wn, half, l31, n0, tx0, ty0, b0);
}

template <int WM, int WN, int MT, int NT>
struct TileCfgB {   // split-bf16 kernel: only the activation tile lives in LDS
    static constexpr int BM = WM * MT * 32, BN = WN * NT * 32, NTHR = WM * WN * 64;
    static constexpr size_t LDS = (size_t)(2 * BM) * 36 * sizeof(float);
};

template <int WM, int WN, int MT, int NT>
static hipError_t set_attr_bf16x3() {
    hipError_t e;
    const int lds = (int)TileCfgB<WM, WN, MT, NT>::LDS;
#define MSR_SET(EPI)                                                                                          \
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm_bf16x3<WM, WN, MT, NT, EPI>),       \
                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds)) != hipSuccess)              \
        return e;
    MSR_SET(EPI_BIAS) MSR_SET(EPI_RES) MSR_SET(EPI_SPADE) MSR_SET(EPI_PARTIAL)
#undef MSR_SET
    return hipSuccess;
}

hipError_t set_attr_bvgpr() {
    hipError_t e;
    if ((e = set_attr_bf16x3<2, 2, 2, 2>()) != hipSuccess) return e;
    return set_attr_bf16x3<2, 1, 1, 2>();
}

template <int WM, int WN, int MT, int NT>
static hipError_t launch_bf16x3(const ConvParams& p, int epi, hipStream_t s) {
    using C = TileCfgB<WM, WN, MT, NT>;
    TileGeom g;
    if (!make_geom(p, C::BM, C::BN, 32, g)) return hipErrorInvalidValue;
    const int grid = g.tiles_mn * (p.ksplit > 1 ? p.ksplit : 1);
    if (p.ksplit > 1) {
        if (!p.partial || (epi != EPI_BIAS && epi != EPI_RES && epi != EPI_SPADE)) return hipErrorInvalidValue;   // no affine form
        conv_igemm_bf16x3<WM, WN, MT, NT, EPI_PARTIAL><<<grid, C::NTHR, C::LDS, s>>>(p, g);
        return finish_splitk(p, epi, s);
    }
    switch (epi) {
        case EPI_BIAS: conv_igemm_bf16x3<WM, WN, MT, NT, EPI_BIAS><<<grid, C::NTHR, C::LDS, s>>>(p, g); break;
        case EPI_RES: conv_igemm_bf16x3<WM, WN, MT, NT, EPI_RES><<<grid, C::NTHR, C::LDS, s>>>(p, g); break;
        case EPI_SPADE: conv_igemm_bf16x3<WM, WN, MT, NT, EPI_SPADE><<<grid, C::NTHR, C::LDS, s>>>(p, g); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_bvgpr(const ConvParams& p, int epi, int tile, hipStream_t s) {
    if (tile == TILE_64x64) return launch_bf16x3<2, 1, 1, 2>(p, epi, s);
    return launch_bf16x3<2, 2, 2, 2>(p, epi, s);
}

}  // namespace msr

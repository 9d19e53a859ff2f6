#include "conv_common.h"
#include "conv_epilogue.h"

namespace msr {

// ------------------------------------------------------------------------------------------------------
// conv_igemm_bf16x3_pp: the halo kernel as a PING-PONG pair of wave groups (512 threads, one workgroup per CU).
//
// With two independent 256-thread workgroups per CU the two waves of a SIMD drift into lockstep: both issue
// their MFMAs together (the matrix pipe is per SIMD, so that is no faster than one wave) and both then sit in
// their LDS phase together, which left the pipe ~60 % busy.  Here the two waves of a SIMD belong to ONE workgroup
// and are held half a K-step apart by the barrier schedule:
//     phase 2t   : group X (waves 0-3)  R(t)  LDS fragment reads, weight staging      | group Y (waves 4-7)  M(t-1)
//     phase 2t+1 : group X              M(t)  48 x v_mfma_f32_16x16x32_bf16, registers | group Y              R(t)
// so every SIMD always has one wave in its matrix segment and one in its memory segment (MI355X_MICROARCH.md,
// "Two waves per SIMD", items 5 and 9).  X owns the top 8 rows of a 16 x 16 pixel tile, Y the bottom 8; both use
// the same 128-channel weight tile.  LDS: input halo (18 x 18 pixels x 32 channels) double-buffered by chunk,
// weight tile double-buffered by K-step, 160-byte rows: 2 * 324 * 160 + 2 * 128 * 160 = 144,640 B.
// Barrier count (s_barrier only counts arrivals; every wave must execute the same number): per K-step each wave
// runs two (after R, after M); group Y runs one extra before its first R and skips the one after its last M of the
// workgroup's last tile: X = 1 + 2 * steps, Y = 1 + 1 + 2 * steps - 1 — equal.  (MSR_WG_BARRIER, conv_common.h.)  On a
// tile's last step Y executes its second barrier AFTER its epilogue (X before): same count, and the two epilogues overlap.
// Hazards (b = barrier at the end of a phase): the weights of step t+1 go to Bs[(t+1)&1] during R(t) of both
// groups (phases 2t, 2t+1); that buffer was last read in R(t-1) (phases 2t-2, 2t-1) and is next read in R(t+1)
// (phases 2t+2, 2t+3).  The halo of chunk c+1 goes to Ah[(c+1)&1] on tap 7 of chunk c.
// ------------------------------------------------------------------------------------------------------
// F16X2 = true is the opt-in 2-term form for the gamma|beta convs (kernels.h PREC_F16X2): operands are split-fp16
// words, the weight's lo half is neither read from LDS nor multiplied: 32 MFMAs and 12 ds_read_b128 per K-step
// instead of 48 and 16.
// MODE 2 (PP_FP8) is the declared non-parity fp8 form (kernels.h PREC_FP8): a chunk row holds 128 one-byte channels,
// a K-step is 128 channels of one tap: 16 block-scaled MFMAs (K = 128 each), same staging and fragment reads.
// MODE 3 (PP_F16C, kernels.h PREC_F16C): fp16 main term + fp8 cross terms.  A chunk row holds [32 x hi f16 | 32 x h8 |
// 32 x l8] (weights: l8 then h8, so that byte t of one pairs with byte t of the other: w_lo*x_hi, w_hi*x_lo).  Every
// K-step runs the 16 f16 MFMAs of its tap (x_hi * w_hi); the lane's 16 bytes at +64 + 16 * (lane >> 4) (the same
// conflict-free read as the bf16 lo half) of an EVEN step and of the following ODD step make one 32-byte operand, and the
// odd step adds 16 block-scaled K = 128 fp8 MFMAs that cover the cross terms of both taps.  In that instruction a lane's
// first 16 bytes are k = 16g.. of the first 64 and its second 16 bytes of the second 64, and k-block b takes its e8m0
// scale from lane group b: blocks 0 / 2 are the even / odd tap's h8 (w: l8) bytes, blocks 1 / 3 their l8 (w: h8) bytes,
// so lane groups 0, 2 carry the scale of the first kind and 1, 3 of the second.  Two MFMA-equivalents per product
// instead of three; per-product error ~2^-15 (the fp8 rounding of a term that is 2^-11 of the product).
enum PpMode : int { PP_BF16X3 = 0, PP_F16X2 = 1, PP_FP8 = 2, PP_F16C = 3 };
// ONE = true: the input has ONE 32-slot chunk (the Cin = 128 convs of the fp8 mode: 128 one-byte channels).  The
// unrolled body of 18 K-steps then covers TWO work items (tiles) of 9 taps each instead of a chunk pair of one tile:
// item B takes the place of "chunk 1" (its halo is staged during A's taps into the other halo buffer, its weights follow
// A's in the weight ring), item A' of the next body the place of "the next tile"; A's epilogue runs between steps 8 and 9.
// The LDS schedule is unchanged.  With an odd number of items the last body computes its item twice (same stores).
template <int EPI, int MODE, bool ONE = false>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv_igemm_bf16x3_pp(const ConvParams p, const TileGeom g) {
    constexpr bool F16X2 = MODE == PP_F16X2;
    constexpr int NTHR = 512, BN = 128, BKC = 32, BKP = 40;
    constexpr int TH = 16, TW = 16, HW = TW + 2, HP = (TH + 2) * HW;          // 324 halo pixels
    constexpr int H_ITEMS = (HP * 8 + NTHR - 1) / NTHR;                        // 6 16-byte items per thread
    static_assert(H_ITEMS == 6, "halo staging is written for 6 items per thread");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const Ah = smem;                       // [2][HP][BKP]
    float* const Bs = smem + 2 * HP * BKP;        // [2][BN][BKP]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // PP_F16C + EPI_SPADE: a private 16 x 36-dword line image per wave behind the tile buffers (epilogue store assembly)
#ifdef MSR_PP_STAMPS
    unsigned* const stage = nullptr;              // the stamp words live there in the diagnostic build
#else
    unsigned* const stage = (MODE == PP_F16C && EPI == EPI_SPADE)
        ? reinterpret_cast<unsigned*>(smem + (2 * HP + 2 * BN) * BKP) + wave * (16 * 36) : nullptr;
#endif
    const int grp = wave >> 2;                    // 0 = X, 1 = Y (wave-uniform, scalar)
    const int wm = (wave >> 1) & 1, wn = wave & 1;

    // Persistent: gridDim.x (a multiple of 8, one workgroup per CU) workgroups walk all tiles.  Workgroups are
    // dealt round-robin over the 8 XCDs, so XCD x owns a contiguous range of logical tiles (as xcd_remap) and its
    // gridDim.x / 8 workgroups take consecutive tiles of that range in every round: the tiles in flight on an XCD
    // share their halo (same pixels, next channel block) and weights in that XCD's L2.
    // With p.ksplit > 1 (fewer tiles than CUs) a work item is (K range, tile): range ks covers chunk pairs
    // [ks * ppi, (ks + 1) * ppi), items are numbered range-major so that neighbours still share their halo.
    const int ksn = p.ksplit > 1 ? p.ksplit : 1;
    const int ppi = ONE ? 1 : (p.Cin / (2 * BKC)) / ksn;                       // chunk pairs per item (ONE: one body = 2 items)
    const unsigned kbytes = (unsigned)ppi * 2u * BKC * 4u;                      // byte offset of one range (input and weights)
    const int items = g.tiles_mn * ksn;
    int slots, cnt, base;
    xcd_tile_range(items, slots, cnt, base);
    int tile = blockIdx.x >> 3;                   // index inside the XCD's range
    if (tile >= cnt) return;

    // per-tile state is scalar: tile origin (pixels, channel block) and its byte offsets in the input / weights
    int n0, tx0, ty0, b0, ks0;
    unsigned h_tile, w_tile;
#define MSR_DECODE(T_, N0_, TX_, TY_, B_, HT_, WT_, KS_)                                          \
    {                                                                                            \
        KS_ = (T_) / g.tiles_mn;                                                                 \
        const int t_ = (T_) - KS_ * g.tiles_mn;                                                  \
        int tn_, tmi_;                                                                           \
        MSR_WALK(g, t_, tn_, tmi_)                                                               \
        TX_ = (tmi_ % g.tiles_x) << 4;                                                           \
        tmi_ /= g.tiles_x;                                                                       \
        TY_ = (tmi_ % g.tiles_y) << 4;                                                           \
        B_ = tmi_ / g.tiles_y;                                                                   \
        N0_ = tn_ * BN;                                                                          \
        HT_ = (unsigned)((B_) * p.in_pb + (TY_) * p.in_py + (TX_) * p.Cin) * 4u + (unsigned)KS_ * kbytes; \
        WT_ = (unsigned)((N0_) * p.Cin) * 4u + (unsigned)KS_ * kbytes;                           \
    }
    MSR_DECODE(base + tile, n0, tx0, ty0, b0, h_tile, w_tile, ks0)

    int h_goff[H_ITEMS], h_loff[H_ITEMS];         // tile-relative byte offsets / LDS float offsets
#pragma unroll
    for (int q = 0; q < H_ITEMS; ++q) {
        int idx = tid + q * NTHR;
        idx = idx < HP * 8 ? idx : HP * 8 - 1;    // items past the end duplicate the last one
        const int hp = idx >> 3, seg = idx & 7;
        const int hy = hp / HW, hx = hp - hy * HW;
        h_goff[q] = (hy * p.in_py + hx * p.Cin + seg * 4) * 4;
        h_loff[q] = hp * BKP + seg * 4;
    }
    int b_goff[2], b_loff[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int idx = tid + q * NTHR;
        const int row = idx >> 3, seg = idx & 7;
        b_goff[q] = (row * p.Cin + seg * 4) * 4;
        b_loff[q] = row * BKP + seg * 4;
    }
    int a_frag[4], b_frag[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a_frag[i] = ((grp * 8 + wm * 4 + i) * HW + (lane & 15)) * BKP + 4 * (lane >> 4);
        b_frag[i] = ((wn * 4 + i) * 16 + (lane & 15)) * BKP + 4 * (lane >> 4);
    }
    f32x4 acc[4][4];
    int wsc[4] = {0x7F7F7F7F, 0x7F7F7F7F, 0x7F7F7F7F, 0x7F7F7F7F};   // PP_FP8: e8m0 weight scales of the wave's 4 x 16 rows

    const unsigned w_tap_bytes = (unsigned)((size_t)p.N * p.Cin * sizeof(float));
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.in), 0, (int)((size_t)p.B * p.in_pb * sizeof(float)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_wt = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.wt), 0, (int)(9u * w_tap_bytes), 0x00020000);
    unsigned h_pair = 0, w_pair = 0;              // byte offsets of the current chunk pair
    unsigned h_next = 0, w_next = 0;              // byte offsets of the NEXT tile (of this one again on the last)
    unsigned h_b = 0, w_b = 0;                    // ONE: the body's second item
    int n0b = 0, tx0b = 0, ty0b = 0, b0b = 0, ksb = 0;

    float4 rh0, rh1, rh2, rh3, rh4, rh5;          // halo of the next chunk in flight
    float4 rw0, rw1;                              // weights of the next K-step in flight
    bf16x8 ah[4], al[4], bh[4], bl[4];            // fragments of the current K-step
    i32x8 qa0, qa1, qa2, qa3, qb0, qb1, qb2, qb3; // ... PP_FP8: the same 32 bytes per lane as ONE 8-register operand
    i32x4 ca0[4], ca1[4], cb0[4], cb1[4];         // ... PP_F16C: the cross-term pieces of an even step and of the odd one after it
    const int asc = ((lane >> 4) & 1) ? 0x74747474 : 0x7F7F7F7F;   // PP_F16C: e8m0 of the activation piece: l8 = x_lo * 2^11 (116), h8 = x_hi (127)
    float4 xpre[4][2], cpre[8];                   // the epilogue's memory operands, requested on step 16 of the last pair
#define MSR_BUFLD(rs, voff, soff) \
    __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, (int)(soff), 0))
#define MSR_LOAD_H_LO(soff)                                                                      \
    {                                                                                            \
        rh0 = MSR_BUFLD(rs_in, h_goff[0], soff); rh1 = MSR_BUFLD(rs_in, h_goff[1], soff);        \
        rh2 = MSR_BUFLD(rs_in, h_goff[2], soff);                                                 \
    }
#define MSR_LOAD_H_HI(soff)                                                                      \
    {                                                                                            \
        rh3 = MSR_BUFLD(rs_in, h_goff[3], soff); rh4 = MSR_BUFLD(rs_in, h_goff[4], soff);        \
        rh5 = MSR_BUFLD(rs_in, h_goff[5], soff);                                                 \
    }
#define MSR_LOAD_H(soff) { MSR_LOAD_H_LO(soff) MSR_LOAD_H_HI(soff) }
#define MSR_WRITE_H_LO(buf)                                                                      \
    {                                                                                            \
        float* h_ = Ah + (buf) * HP * BKP;                                                       \
        *reinterpret_cast<float4*>(h_ + h_loff[0]) = rh0; *reinterpret_cast<float4*>(h_ + h_loff[1]) = rh1; \
        *reinterpret_cast<float4*>(h_ + h_loff[2]) = rh2;                                        \
    }
#define MSR_WRITE_H_HI(buf)                                                                      \
    {                                                                                            \
        float* h_ = Ah + (buf) * HP * BKP;                                                       \
        *reinterpret_cast<float4*>(h_ + h_loff[3]) = rh3; *reinterpret_cast<float4*>(h_ + h_loff[4]) = rh4; \
        *reinterpret_cast<float4*>(h_ + h_loff[5]) = rh5;                                        \
    }
#define MSR_WRITE_H(buf) { MSR_WRITE_H_LO(buf) MSR_WRITE_H_HI(buf) }
// weights of K-step U of a chunk pair, relative to the pair's first chunk
#define MSR_WOFF(U) (((U) / 9) * (BKC * 4) + (unsigned)((U) % 9) * w_tap_bytes)
#define MSR_LOAD_B(soff)                                                                         \
    { rw0 = MSR_BUFLD(rs_wt, b_goff[0], soff); rw1 = MSR_BUFLD(rs_wt, b_goff[1], soff); }
#define MSR_WRITE_B(buf)                                                                         \
    {                                                                                            \
        float* b_ = Bs + (buf) * BN * BKP;                                                       \
        *reinterpret_cast<float4*>(b_ + b_loff[0]) = rw0; *reinterpret_cast<float4*>(b_ + b_loff[1]) = rw1; \
    }
// R(T): memory segment of K-step T (0..17 within the pair, compile time).  The staging never stops: on the last
// pair of a tile (LASTP) the steps past its end are the first steps of the NEXT tile (weights of its steps 0 and
// 1, halo of its chunk 0), so no load or LDS write sits under a run-time condition; on the last tile of the
// workgroup "next" is the tile itself and the staged data is simply never read.
#define MSR_R(T, LASTP)                                                                          \
    {                                                                                            \
        MSR_WRITE_B(((T) + 1) & 1);                                                              \
        if constexpr (ONE) {                                                                     \
            if ((T) + 2 >= 18) MSR_LOAD_B(w_next + (unsigned)((T) + 2 - 18) * w_tap_bytes)       \
            else if ((T) + 2 >= 9) MSR_LOAD_B(w_b + (unsigned)((T) + 2 - 9) * w_tap_bytes)       \
            else MSR_LOAD_B(w_tile + (unsigned)((T) + 2) * w_tap_bytes);                         \
            if ((T) == 1) MSR_LOAD_H(h_b)                                                        \
            if ((T) == 10) MSR_LOAD_H(h_next)                                                    \
        } else {                                                                                 \
            if ((LASTP) && (T) + 2 >= 18) MSR_LOAD_B(w_next + MSR_WOFF((T) + 2 - 18))            \
            else MSR_LOAD_B(w_tile + w_pair + MSR_WOFF((T) + 2));                                \
            if ((T) % 9 == 1) {                                                                  \
                if ((LASTP) && (T) >= 9) MSR_LOAD_H(h_next)                                      \
                else MSR_LOAD_H(h_tile + h_pair + ((T) / 9 + 1) * BKC * 4);                      \
            }                                                                                    \
        }                                                                                        \
        /* the halo of the next chunk goes to LDS in two halves (taps 6 and 7): all six stores in one R make that   \
           segment longer than the partner's matrix segment (1060 vs 840 cycles) */              \
        if ((T) % 9 == 6) MSR_WRITE_H_LO((((T) / 9) & 1) ^ 1);                                   \
        if ((T) % 9 == 7) MSR_WRITE_H_HI((((T) / 9) & 1) ^ 1);                                   \
        const float* a_ = Ah + (((T) / 9) & 1) * HP * BKP + ((((T) % 9) / 3) * HW + (((T) % 9) % 3)) * BKP; \
        const float* b_ = Bs + ((T) & 1) * BN * BKP;                                             \
        if constexpr (MODE == PP_FP8) {                                                          \
            /* the K = 128 MFMA takes 8 consecutive registers per operand: both 16-byte halves into one vector */ \
            MSR_RD8(qa0, a_ + a_frag[0]) MSR_RD8(qa1, a_ + a_frag[1]) MSR_RD8(qa2, a_ + a_frag[2]) MSR_RD8(qa3, a_ + a_frag[3]) \
            MSR_RD8(qb0, b_ + b_frag[0]) MSR_RD8(qb1, b_ + b_frag[1]) MSR_RD8(qb2, b_ + b_frag[2]) MSR_RD8(qb3, b_ + b_frag[3]) \
        } else if constexpr (MODE == PP_F16C) {                                                  \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                      \
                ah[i] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[i]);                        \
                bh[i] = *reinterpret_cast<const bf16x8*>(b_ + b_frag[i]);                        \
                if (((T) & 1) == 0) {                                                            \
                    ca0[i] = *reinterpret_cast<const i32x4*>(a_ + a_frag[i] + 16);               \
                    cb0[i] = *reinterpret_cast<const i32x4*>(b_ + b_frag[i] + 16);               \
                } else {                                                                         \
                    ca1[i] = *reinterpret_cast<const i32x4*>(a_ + a_frag[i] + 16);               \
                    cb1[i] = *reinterpret_cast<const i32x4*>(b_ + b_frag[i] + 16);               \
                }                                                                                \
            }                                                                                    \
        } else {                                                                                 \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                      \
                ah[i] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[i]);                        \
                al[i] = *reinterpret_cast<const bf16x8*>(a_ + a_frag[i] + 16);                   \
                bh[i] = *reinterpret_cast<const bf16x8*>(b_ + b_frag[i]);                        \
                if constexpr (!F16X2) bl[i] = *reinterpret_cast<const bf16x8*>(b_ + b_frag[i] + 16); \
            }                                                                                    \
        }                                                                                        \
    }
// M(T): matrix segment, registers only (weights as the row operand: D[channel][pixel])
#define MSR_RD8(dst, ptr)                                                                        \
    {                                                                                            \
        const i32x4 lo_ = *reinterpret_cast<const i32x4*>(ptr);                                  \
        const i32x4 hi_ = *reinterpret_cast<const i32x4*>((ptr) + 16);                           \
        dst = __builtin_shufflevector(lo_, hi_, 0, 1, 2, 3, 4, 5, 6, 7);                         \
    }
#define MSR_MF8(J, WQ)                                                                           \
    acc[0][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(WQ, qa0, acc[0][J], 0, 1, 0, wsc[J], 0, 0x7F7F7F7F); \
    acc[1][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(WQ, qa1, acc[1][J], 0, 1, 0, wsc[J], 0, 0x7F7F7F7F); \
    acc[2][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(WQ, qa2, acc[2][J], 0, 1, 0, wsc[J], 0, 0x7F7F7F7F); \
    acc[3][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(WQ, qa3, acc[3][J], 0, 1, 0, wsc[J], 0, 0x7F7F7F7F);
#define MSR_F16(v) __builtin_bit_cast(f16x8, v)
#define MSR_CAT8(lo, hi) __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7)
#define MSR_M(T)                                                                                 \
    if constexpr (MODE == PP_F16C) {                                                             \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                          \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                        \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(MSR_F16(bh[j]), MSR_F16(ah[i]), acc[i][j], 0, 0, 0); \
        }                                                                                        \
        if (((T) & 1) == 1) {                                                                    \
            /* the cross MFMA of an accumulator 16 instructions after its main one: no dependent-issue stall */ \
            __builtin_amdgcn_sched_barrier(0);                                                   \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                      \
                const i32x8 wq_ = MSR_CAT8(cb0[j], cb1[j]);                                      \
                _Pragma("unroll") for (int i = 0; i < 4; ++i)                                    \
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wq_, MSR_CAT8(ca0[i], ca1[i]), acc[i][j], \
                                                                                 0, 0, 0, wsc[j], 0, asc); \
            }                                                                                    \
        }                                                                                        \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                            \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(acc[i][j]));     \
    } else if constexpr (MODE == PP_FP8) {                                                       \
        /* weights fp8 e4m3 (row operand, per-channel e8m0 scale in wsc[j]) x activations bf8 e5m2 (unit scale) */ \
        MSR_MF8(0, qb0) MSR_MF8(1, qb1) MSR_MF8(2, qb2) MSR_MF8(3, qb3)                          \
        /* pin the accumulators here: without a use in this segment LLVM sinks the whole MFMA chain of the last chunk  \
           pair into the epilogue (per output row) and keeps 18 steps of fragments alive in scratch */ \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                            \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(acc[i][j]));     \
    } else if constexpr (F16X2) {                                                                \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                          \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                        \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(MSR_F16(bh[j]), MSR_F16(al[i]), acc[i][j], 0, 0, 0); \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                        \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(MSR_F16(bh[j]), MSR_F16(ah[i]), acc[i][j], 0, 0, 0); \
        }                                                                                        \
    } else {                                                                                     \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                          \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                        \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[j], al[i], acc[i][j], 0, 0, 0); \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                        \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl[j], ah[i], acc[i][j], 0, 0, 0); \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                        \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[j], ah[i], acc[i][j], 0, 0, 0); \
        }                                                                                        \
    }
// Diagnostic build only (-DMSR_PP_STAMPS, tools/gpu_pp_stamps.py): s_memtime stamps of waves 0 (X) and 4 (Y) of one
// workgroup around the segments of one chunk pair, kept in the LDS words behind the product's 144,640 bytes.
#ifdef MSR_PP_STAMPS
#define MSR_STAMP()                                                                              \
    if (dbg_on && lane == 0 && (wave & 3) == 0) dbg[(wave >> 2) * 1024 + dbg_n++] = (unsigned)__builtin_amdgcn_s_memtime();
#else
#define MSR_STAMP()
#endif
#define MSR_STEP(T, LASTP)                                                                       \
    {                                                                                            \
        MSR_STAMP()                                                                              \
        MSR_R(T, LASTP)                                                                          \
        if constexpr (ONE) {                                                                     \
            if ((T) == 7 && MODE != PP_FP8) halo16_epilogue_load<EPI>(p, xpre, cpre, wm, wn, lane, n0, tx0, ty0 + grp * 8, b0); \
            if ((T) == 16 && MODE != PP_FP8) halo16_epilogue_load<EPI>(p, xpre, cpre, wm, wn, lane, n0b, tx0b, ty0b + grp * 8, b0b); \
        } else {                                                                                 \
            if ((LASTP) && (T) == 16 && EPI != EPI_PARTIAL && MODE != PP_FP8 && MODE != PP_F16C) halo16_epilogue_load<EPI>(p, xpre, cpre, wm, wn, lane, n0, tx0, ty0 + grp * 8, b0); \
        }                                                                                        \
        MSR_STAMP()                                                                              \
        MSR_WG_BARRIER()                                                                         \
        MSR_STAMP()                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        MSR_M(T)                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        MSR_STAMP()                                                                              \
        /* Y's M on the workgroup's very last step has no partner segment.  On a tile's last step (not ONE) group Y    \
           postpones this barrier until after its epilogue (below the pair), so that both groups' epilogues share ONE \
           barrier interval */                                                                   \
        if (ONE || !((LASTP) && (T) == 17)) MSR_WG_BARRIER()                                     \
        else if (grp == 0) MSR_WG_BARRIER()                                                      \
        if constexpr (ONE) {                                                                     \
            if ((T) == 8) {   /* item A is complete: its epilogue, fresh accumulators, item B's weight scales */ \
                if constexpr (MODE == PP_FP8) halo16_epilogue_load<EPI>(p, xpre, cpre, wm, wn, lane, n0, tx0, ty0 + grp * 8, b0); \
                halo16_epilogue<EPI>(p, ge, acc, wm, wn, lane, n0, tx0, ty0 + grp * 8, b0, xpre, cpre); \
                _Pragma("unroll") for (int i = 0; i < 4; ++i)                                    \
                    _Pragma("unroll") for (int j = 0; j < 4; ++j)                                \
                        _Pragma("unroll") for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;        \
                if constexpr (MODE == PP_FP8) {                                                  \
                    _Pragma("unroll") for (int j = 0; j < 4; ++j) wsc[j] = p.wexp[n0b + wn * 64 + j * 16 + (lane & 15)]; \
                }                                                                                \
            }                                                                                    \
        }                                                                                        \
    }
#define MSR_PAIR(LASTP)                                                                          \
    MSR_STEP(0, LASTP) MSR_STEP(1, LASTP) MSR_STEP(2, LASTP) MSR_STEP(3, LASTP) MSR_STEP(4, LASTP) \
    MSR_STEP(5, LASTP) MSR_STEP(6, LASTP) MSR_STEP(7, LASTP) MSR_STEP(8, LASTP) MSR_STEP(9, LASTP) \
    MSR_STEP(10, LASTP) MSR_STEP(11, LASTP) MSR_STEP(12, LASTP) MSR_STEP(13, LASTP)              \
    MSR_STEP(14, LASTP) MSR_STEP(15, LASTP) MSR_STEP(16, LASTP) MSR_STEP(17, LASTP)

#ifdef MSR_PP_STAMPS
    unsigned* dbg = reinterpret_cast<unsigned*>(smem + (2 * HP + 2 * BN) * BKP);
    int dbg_n = 0;
    bool dbg_on = false;
#endif
    // prologue of the workgroup's first tile: halo of chunk 0 and the weights of step 0 into LDS, the weights of
    // step 1 stay in flight
    MSR_LOAD_H(h_tile);
    MSR_LOAD_B(w_tile + MSR_WOFF(0));
    MSR_WRITE_H(0);
    MSR_WRITE_B(0);
    MSR_LOAD_B(w_tile + MSR_WOFF(1));
    MSR_WG_BARRIER()
    if (grp == 1) MSR_WG_BARRIER()                // Y starts half a step late (phase 0 is X's R(0) alone)
    TileGeom ge = g;                              // the epilogue numbers its moment slabs by 8-row tiles
    ge.th_l = 3;
    ge.tiles_y = g.tiles_y * 2;
#ifdef MSR_PP_STAMPS
    unsigned tstamp[20];
    int tstamp_n = 0;
#endif
    for (;;) {
#ifdef MSR_PP_STAMPS
        if (tstamp_n < 20) tstamp[tstamp_n++] = (unsigned)__builtin_amdgcn_s_memtime();      // coarse: one stamp per tile
#endif
        const int tnext = ONE ? tile + 2 * slots : tile + slots;
        const bool has_next = tnext < cnt;
        int n0n, tx0n, ty0n, b0n, ks0n;
        MSR_DECODE(base + (has_next ? tnext : tile), n0n, tx0n, ty0n, b0n, h_next, w_next, ks0n)
        if constexpr (ONE) {
            const int tb = tile + slots < cnt ? tile + slots : tile;      // no second item left: item A again
            MSR_DECODE(base + tb, n0b, tx0b, ty0b, b0b, h_b, w_b, ksb)
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
        if constexpr (MODE == PP_FP8) {
#pragma unroll
            for (int j = 0; j < 4; ++j) wsc[j] = p.wexp[n0 + wn * 64 + j * 16 + (lane & 15)];
        }
        if constexpr (MODE == PP_F16C) {    // byte 0 = e8m0 of the channel's w_lo pieces (even lane groups), byte 1 = of its w_hi pieces
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int w_ = p.wexp[n0 + wn * 64 + j * 16 + (lane & 15)];
                wsc[j] = ((((lane >> 4) & 1) ? (w_ >> 8) : w_) & 0xFF) * 0x01010101;
            }
        }
        h_pair = 0;
        w_pair = 0;
        for (int pr = 0; pr < ppi - 1; ++pr) {
#ifdef MSR_PP_STAMPS
            dbg_on = blockIdx.x == 8 && pr == 2 && dbg_n == 0;
#endif
            MSR_PAIR(false)
#ifdef MSR_PP_STAMPS
            dbg_on = false;
#endif
            h_pair += 2 * BKC * 4;
            w_pair += 2 * BKC * 4;
        }
        MSR_PAIR(true)
        // Both groups run their epilogue in the SAME barrier interval: X after the barrier that follows its last M (beside
        // its R(0) of the next tile), Y right after its last M, BEFORE that barrier.  (Each group used to run it after the
        // barrier: X's epilogue then faced only Y's last M and Y's only X's first M of the next tile, i.e. the two
        // epilogues — ~10k cycles each with their loads and stores — ran one after the other: a gamma|beta tile took 87k
        // cycles for 58k of K loop, tools/gpu_pp_stamps_gb.py.)  Its stores are not waited for.
        // PP_FP8: the scaled MFMA does not accumulate in place under register pressure, so its epilogue operands are
        // not held across the last K-steps but requested here
        if constexpr (ONE) {       // the body's second item
            if constexpr (MODE == PP_FP8) halo16_epilogue_load<EPI>(p, xpre, cpre, wm, wn, lane, n0b, tx0b, ty0b + grp * 8, b0b);
            halo16_epilogue<EPI>(p, ge, acc, wm, wn, lane, n0b, tx0b, ty0b + grp * 8, b0b, xpre, cpre);
        } else {
            if constexpr (MODE == PP_FP8 || MODE == PP_F16C) halo16_epilogue_load<EPI>(p, xpre, cpre, wm, wn, lane, n0, tx0, ty0 + grp * 8, b0);
            if constexpr (EPI == EPI_PARTIAL) halo16_epilogue_partial(p, acc, wm, wn, lane, n0, tx0, ty0 + grp * 8, b0, ks0);
            else halo16_epilogue<EPI>(p, ge, acc, wm, wn, lane, n0, tx0, ty0 + grp * 8, b0, xpre, cpre, stage);
            if (grp == 1 && has_next) MSR_WG_BARRIER()        // Y's barrier of the tile's last step (see MSR_STEP)
        }
        if (!has_next) break;
        tile = tnext;
        n0 = n0n; tx0 = tx0n; ty0 = ty0n; b0 = b0n; ks0 = ks0n;
        h_tile = h_next;
        w_tile = w_next;
    }
#ifdef MSR_PP_STAMPS
    if (blockIdx.x == 8 && lane == 0 && (wave & 3) == 0) {
        for (int k = 0; k + 1 < tstamp_n; ++k) printf("wave %d tile %2d: %6u cycles\n", wave, k, tstamp[k + 1] - tstamp[k]);
        const unsigned* d = dbg + (wave >> 2) * 1024;
        for (int k = 0; k + 3 < dbg_n; k += 4)
            printf("wave %d step %2d: R %4u  barrier %4u  M %4u  barrier+next %4u cycles\n", wave, k / 4, d[k + 1] - d[k],
                   d[k + 2] - d[k + 1], d[k + 3] - d[k + 2], k + 4 < dbg_n ? d[k + 4] - d[k + 3] : 0u);
    }
#endif
#undef MSR_STAMP
#undef MSR_DECODE
#undef MSR_BUFLD
#undef MSR_LOAD_H
#undef MSR_WRITE_H
#undef MSR_WRITE_H_LO
#undef MSR_WRITE_H_HI
#undef MSR_LOAD_H_LO
#undef MSR_LOAD_H_HI
#undef MSR_WOFF
#undef MSR_LOAD_B
#undef MSR_WRITE_B
#undef MSR_R
#undef MSR_M
#undef MSR_F16
#undef MSR_CAT8
#undef MSR_RD8
#undef MSR_MF8
#undef MSR_STEP
#undef MSR_PAIR
}

#ifdef MSR_PP_STAMPS
static constexpr size_t PP_LDS = (size_t)(2 * 324 + 2 * 128) * 40 * sizeof(float) + 8192;   // + the stamp words
#else
static constexpr size_t PP_LDS = (size_t)(2 * 324 + 2 * 128) * 40 * sizeof(float);
#endif
// PP_F16C + EPI_SPADE launches: + 8 waves x 16 lines x 36 dwords of epilogue store assembly = 163,072 B of the CU's 163,840
#ifdef MSR_PP_STAMPS
static constexpr size_t PP_STAGE_LDS = 0;
#else
static constexpr size_t PP_STAGE_LDS = (size_t)8 * 16 * 36 * sizeof(unsigned);
#endif

hipError_t set_attr_pp() {
    hipError_t e;
#define MSR_SETPP(EPI, ...)                                                                                   \
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm_bf16x3_pp<EPI, __VA_ARGS__>),       \
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)PP_LDS)) != hipSuccess)      \
        return e;
    MSR_SETPP(EPI_BIAS, PP_BF16X3) MSR_SETPP(EPI_RES, PP_BF16X3) MSR_SETPP(EPI_SPADE, PP_BF16X3)
    MSR_SETPP(EPI_SPADE, PP_F16X2) MSR_SETPP(EPI_PARTIAL, PP_BF16X3)
    MSR_SETPP(EPI_BIAS, PP_FP8) MSR_SETPP(EPI_RES, PP_FP8) MSR_SETPP(EPI_SPADE, PP_FP8)
    MSR_SETPP(EPI_BIAS, PP_FP8, true) MSR_SETPP(EPI_RES, PP_FP8, true) MSR_SETPP(EPI_SPADE, PP_FP8, true)
    MSR_SETPP(EPI_BIAS, PP_F16C) MSR_SETPP(EPI_RES, PP_F16C) MSR_SETPP(EPI_PARTIAL, PP_F16C)
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm_bf16x3_pp<EPI_SPADE, PP_F16C>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)(PP_LDS + PP_STAGE_LDS))) != hipSuccess)
        return e;
#undef MSR_SETPP
    return hipSuccess;
}

// One launch of the ping-pong kernel's MODE form for a runtime epilogue (the f16c SPADE epilogue assembles its stores in
// LDS behind the tile buffers: PP_STAGE_LDS more).
template <int MODE, bool ONE = false>
static hipError_t launch_pp_epi(const ConvParams& p, const TileGeom& g, int epi, int grid, hipStream_t s) {
    switch (epi) {
        case EPI_BIAS: conv_igemm_bf16x3_pp<EPI_BIAS, MODE, ONE><<<grid, 512, PP_LDS, s>>>(p, g); break;
        case EPI_RES: conv_igemm_bf16x3_pp<EPI_RES, MODE, ONE><<<grid, 512, PP_LDS, s>>>(p, g); break;
        case EPI_SPADE:
            conv_igemm_bf16x3_pp<EPI_SPADE, MODE, ONE><<<grid, 512, MODE == PP_F16C ? PP_LDS + PP_STAGE_LDS : PP_LDS, s>>>(p, g);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_pp(const ConvParams& p, int epi, hipStream_t s) {
    TileGeom g;
    if (!make_geom(p, 256, 128, 32, g)) return hipErrorInvalidValue;
    const bool one = p.prec == PREC_FP8 && p.Cin == 32;            // one 128-byte chunk: two tiles per unrolled body
    if (!one) conv_walk(g);
    if (g.tb != 1 || g.th_l != 4 || g.tw_l != 4 || p.stride != 1 || p.KH != 3 || p.KW != 3 || (!one && p.Cin % 64))
        return hipErrorInvalidValue;
    const int ksn = p.ksplit > 1 ? p.ksplit : 1;
    if (!one && (p.Cin / 64) % ksn) return hipErrorInvalidValue;  // every K range is a whole number of chunk pairs
    if (one && ksn > 1) return hipErrorInvalidValue;
    if ((size_t)p.B * p.in_pb * sizeof(float) >= ((size_t)1 << 31)) return hipErrorInvalidValue;   // buffer descriptor range
    const int grid = persistent_grid(g.tiles_mn * ksn);       // one workgroup per CU (144 KB of LDS each)
    if (!grid) return hipErrorInvalidValue;
    if (ksn > 1) {
        // few tiles: K ranges fill the chip, raw accumulators go to the split-K workspace, one more pass finishes
        if (!p.partial || (p.prec != PREC_BF16X3 && p.prec != PREC_F16C)) return hipErrorInvalidValue;     // K ranges: 3-term and f16c forms
        if (epi != EPI_BIAS && epi != EPI_RES && epi != EPI_SPADE) return hipErrorInvalidValue;            // no affine form
        if (p.prec == PREC_F16C) {
            if (!p.wexp) return hipErrorInvalidValue;
            conv_igemm_bf16x3_pp<EPI_PARTIAL, PP_F16C><<<grid, 512, PP_LDS, s>>>(p, g);
        } else {
            conv_igemm_bf16x3_pp<EPI_PARTIAL, PP_BF16X3><<<grid, 512, PP_LDS, s>>>(p, g);
        }
        return finish_splitk(p, epi, s);
    }
    if (p.prec == PREC_F16X2) {
        if (epi != EPI_SPADE) return hipErrorInvalidValue;     // the 2-term form exists for the gamma|beta convs only
        conv_igemm_bf16x3_pp<EPI_SPADE, PP_F16X2><<<grid, 512, PP_LDS, s>>>(p, g);
        return hipGetLastError();
    }
    if ((p.prec == PREC_F16C || p.prec == PREC_FP8) && !p.wexp) return hipErrorInvalidValue;
    if (p.prec == PREC_F16C) return launch_pp_epi<PP_F16C>(p, g, epi, grid, s);
    if (p.prec == PREC_FP8) return one ? launch_pp_epi<PP_FP8, true>(p, g, epi, grid, s) : launch_pp_epi<PP_FP8>(p, g, epi, grid, s);
    return launch_pp_epi<PP_BF16X3>(p, g, epi, grid, s);
}

}  // namespace msr

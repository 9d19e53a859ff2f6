// The two epilogue families of the conv kernels: the 32x32 C/D map (conv_generic, conv_bvgpr, conv_halo SH = 0) and the
// 16x16 map (conv_halo SH = 1, conv_pp).  __forceinline__ templates, instantiated inside each kernel.
#pragma once
#include "conv_common.h"

namespace msr {

// ------------------------------------------------------------------------------------------------------
// Epilogue shared by the fp32 and the split-bf16 kernels.
// C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8*(reg >> 2) + 4*(lane >> 5).
// Per m-tile the 16 rows a lane owns are handled in two phases — (1) addresses and ALL global loads (the tensor
// being normalised / the residual), (2) arithmetic and stores — so the loads of a tile are in flight together
// instead of one load-wait-use chain per row.  Rows outside the batch read a clamped (valid) address and are
// only masked at the store.
// ------------------------------------------------------------------------------------------------------
template <int WM, int WN, int MT, int NT, int EPI, bool SPLIT, int RB>
__device__ __forceinline__ void conv_epilogue_body(const ConvParams& p, const TileGeom& g, f32x16 (&acc)[MT][NT],
                                                   int wm, int wn, int half, int l31, int n0, int tx0, int ty0,
                                                   int b0, int stat_tile) {
    const int twm = (1 << g.tw_l) - 1, thm = (1 << g.th_l) - 1;
    constexpr int NCH = EPI == EPI_SPADE ? NT / 2 : NT;
    float cb0[NCH], cb1[NCH], cmean[NCH], cstd[NCH];
    int ccol[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        if constexpr (EPI == EPI_SPADE) {
            const int colg = n0 + (wn * NT + 2 * j) * 32 + l31;   // gamma column; its beta twin is +32
            ccol[j] = (n0 + wn * NT * 32) / 2 + j * 32 + l31;    // channel
            cb0[j] = p.bias[colg];
            cb1[j] = p.bias[colg + 32];
            cmean[j] = p.mean[ccol[j]];
            cstd[j] = SPLIT ? 1.f / p.stdv[ccol[j]] : p.stdv[ccol[j]];   // bf16x3: multiply by 1/sigma
        } else {
            ccol[j] = n0 + (wn * NT + j) * 32 + l31;
            cb0[j] = p.bias[ccol[j]];
            cb1[j] = cmean[j] = cstd[j] = 0.f;
            if constexpr (EPI == EPI_AFFINE) cb1[j] = p.scale ? p.scale[ccol[j]] : 1.f;
        }
    }
    // fused output moments (EPI_BIAS / EPI_RES): shifted sums per lane and column, shift = the lane's first value
    float st_v0[NT], st_s1[NT], st_s2[NT], st_n = 0.f;
#pragma unroll
    for (int n = 0; n < NT; ++n) st_v0[n] = st_s1[n] = st_s2[n] = 0.f;
#pragma unroll
    for (int mr = 0; mr < MT * (16 / RB); ++mr) {
        const int m = mr / (16 / RB), r0 = (mr % (16 / RB)) * RB;   // RB rows of m-tile m per batch
        int ooff[RB];
        bool ok[RB];
        float xin[RB][NCH];
        // phase 1: addresses and loads
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            const int r = r0 + q;
            const int row = (wm * MT + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int tx = row & twm, ty = (row >> g.tw_l) & thm, tbi = row >> (g.tw_l + g.th_l);
            int bb = b0 + tbi;
            ok[q] = tbi < g.tb && bb < p.B;
            bb = bb < p.B ? bb : p.B - 1;
            const int y = ty0 + ty, x = tx0 + tx;
            ooff[q] = p.out_off + bb * p.out_pb + y * p.out_py + x * p.out_px;
            if constexpr (EPI == EPI_SPADE || EPI == EPI_RES) {
                const float* arow = p.aux + (size_t)bb * p.aux_pb + (y >> p.aux_shift) * p.aux_py +
                                    (x >> p.aux_shift) * p.aux_px;
#pragma unroll
                for (int j = 0; j < NCH; ++j) xin[q][j] = arow[ccol[j]];
            }
        }
        // phase 2: arithmetic and stores
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            const int r = r0 + q;
            float* orow = p.out + ooff[q];
            if constexpr (EPI == EPI_SPADE) {
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    const float gam = acc[m][2 * j][r] + cb0[j];
                    const float bet = acc[m][2 * j + 1][r] + cb1[j];
                    const float normalized = SPLIT ? (xin[q][j] - cmean[j]) * cstd[j] : (xin[q][j] - cmean[j]) / cstd[j];
                    float v = gam * normalized + bet;
                    v = v >= 0.f ? v : v * p.slope;
                    if constexpr (SPLIT) {
                        // lanes 0..31 of a half-wave hold the 32 channels of ONE chunk of this pixel: pair up
                        // neighbouring lanes so that every lane still issues one 4-byte store
                        unsigned hi, lo;
                        msr_split_bf16(v, hi, lo);
                        const unsigned nhi = lane_xor1(hi), nlo = lane_xor1(lo);
                        unsigned* chunk = reinterpret_cast<unsigned*>(orow) + (ccol[j] & ~31);
                        const unsigned word = (l31 & 1) ? (nlo | (lo << 16)) : (hi | (nhi << 16));
                        if (ok[q]) chunk[((l31 & 1) ? 16 : 0) + (l31 >> 1)] = word;
                    } else {
                        if (ok[q]) orow[ccol[j]] = v;
                    }
                }
            } else {
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    float v = acc[m][n][r] + cb0[n];
                    if constexpr (EPI == EPI_AFFINE) {
                        v = acc[m][n][r] * cb1[n] + cb0[n];
                        v = p.act == 1 ? (v <= 0.f ? 0.f : v) : (p.act == 2 ? (v >= 0.f ? v : v * p.slope) : v);    // relu keeps NaN (fmaxf drops it)
                    }
                    if constexpr (EPI == EPI_RES) v += xin[q][n];
                    if (ok[q]) orow[ccol[n]] = v;
                    if (mr == 0 && q == 0) st_v0[n] = v;
                    const float d = ok[q] ? v - st_v0[n] : 0.f;
                    st_s1[n] += d;
                    st_s2[n] += d * d;
                }
                st_n += ok[q] ? 1.f : 0.f;
            }
        }
    }
    if constexpr (EPI == EPI_BIAS || EPI == EPI_RES) {
        if (p.stat_partial) {
            // lane -> (count, mean, M2); lanes l and l ^ 32 hold the same columns for different rows: Chan-combine
            const int slab = (stat_tile * WM + wm);
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const float cnt = st_n;
                const float inv = cnt > 0.f ? 1.f / cnt : 0.f;
                float mean = st_v0[n] + st_s1[n] * inv;
                float m2 = st_s2[n] - st_s1[n] * st_s1[n] * inv;
                const float ocnt = __shfl_xor(cnt, 32), omean = __shfl_xor(mean, 32), om2 = __shfl_xor(m2, 32);
                const float tot = cnt + ocnt;
                if (tot > 0.f) {
                    const float delta = omean - mean;
                    m2 = m2 + om2 + delta * delta * (cnt * ocnt / tot);
                    mean = mean + delta * (ocnt / tot);
                }
                if (half == 0) {
                    float* o = p.stat_partial + (size_t)slab * 3 * p.N + ccol[n];
                    o[0] = tot;
                    o[p.N] = mean;
                    o[2 * p.N] = m2 > 0.f ? m2 : 0.f;
                }
            }
        }
    }
}

template <int WM, int WN, int MT, int NT, int EPI, int RB = 16>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, const TileGeom& g, f32x16 (&acc)[MT][NT], int ks,
                                              int wm, int wn, int half, int l31, int n0, int tx0, int ty0, int b0) {
    // m-tile index of this workgroup (slab row of the fused output moments)
    const int stat_tile = ((b0 / g.tb) * g.tiles_y + (ty0 >> g.th_l)) * g.tiles_x + (tx0 >> g.tw_l);
    if constexpr (EPI == EPI_PARTIAL) {
        const int twm = (1 << g.tw_l) - 1, thm = (1 << g.th_l) - 1;
        float* pbase = p.partial + (size_t)ks * ((size_t)p.B * p.Hout * p.Wout * p.N);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (wm * MT + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int tx = row & twm, ty = (row >> g.tw_l) & thm, tbi = row >> (g.tw_l + g.th_l);
                const int bb = b0 + tbi;
                if (tbi >= g.tb || bb >= p.B) continue;
                float* orow = pbase + (((size_t)bb * p.Hout + ty0 + ty) * p.Wout + tx0 + tx) * p.N;
#pragma unroll
                for (int n = 0; n < NT; ++n) orow[n0 + (wn * NT + n) * 32 + l31] = acc[m][n][r];
            }
        }
    } else if constexpr (EPI == EPI_SPADE) {
        if (p.out_split) conv_epilogue_body<WM, WN, MT, NT, EPI, true, RB>(p, g, acc, wm, wn, half, l31, n0, tx0, ty0, b0, stat_tile);
        else conv_epilogue_body<WM, WN, MT, NT, EPI, false, RB>(p, g, acc, wm, wn, half, l31, n0, tx0, ty0, b0, stat_tile);
    } else {
        conv_epilogue_body<WM, WN, MT, NT, EPI, false, RB>(p, g, acc, wm, wn, half, l31, n0, tx0, ty0, b0, stat_tile);
    }
}

// ------------------------------------------------------------------------------------------------------
// Epilogue of the 16x16x32 halo kernels.  They issue the MFMA with the WEIGHT fragment as the row operand, i.e.
// they accumulate the transposed tile D[channel][pixel]: column = lane & 15 = pixel, row = 4 * (lane >> 4) + reg =
// channel, so a lane holds FOUR CONSECUTIVE CHANNELS of one pixel in the four registers of a sub-tile and every
// global access below is 16 bytes (8 for the split-bf16 halves).  A dword access costs the memory pipeline the
// same 16 cycles per wave-instruction as a 16-byte one: with one workgroup per CU the epilogue is exposed, and the
// dword form of it was 10-30 % of the short-K layers.
// A wave owns tile rows 4*wm .. 4*wm+3 (sub-tile i = one row of 16 pixels) and 64 output columns (sub-tile j = 16
// columns): lane (px, cg) holds pixel x = tx0 + px of each of its four rows.  The tile is always interior
// (tb == 1, r >= 16): nothing is masked.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 f4(const f32x4& v) { return make_float4(v[0], v[1], v[2], v[3]); }

// Everything the epilogue reads from memory, so that the ping-pong kernel can request it two K-steps before the end
// of a tile's main loop (the staging registers are idle by then) instead of paying the latency after it:
//   EPI_SPADE: xin[i][jj] = channels ch0 + 16*jj + 4*cg + {0..3} of x at pixel (y0 + i, x);
//              cv = {gamma bias, beta bias, mean, sigma} x {jj = 0, 1}
//   others   : cv[j] = bias of columns n0 + 64*wn + 16*j + 4*cg + {0..3}
template <int EPI>
__device__ __forceinline__ void halo16_epilogue_load(const ConvParams& p, float4 (&xin)[4][2], float4 (&cv)[8], int wm,
                                                     int wn, int lane, int n0, int tx0, int ty0, int b0) {
    const int px = lane & 15, cg = lane >> 4;
    if constexpr (EPI == EPI_SPADE) {
        const int x = tx0 + px, y0 = ty0 + wm * 4;
        const int ch0 = (n0 + wn * 64) >> 1;
        const float* const abase = p.aux + (size_t)b0 * p.aux_pb + (x >> p.aux_shift) * p.aux_px + ch0 + 4 * cg;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* arow = abase + ((y0 + i) >> p.aux_shift) * p.aux_py;
            xin[i][0] = *reinterpret_cast<const float4*>(arow);
            xin[i][1] = *reinterpret_cast<const float4*>(arow + 16);
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int colg = n0 + wn * 64 + jj * 16 + 4 * cg;
            const int ch = ch0 + jj * 16 + 4 * cg;
            cv[jj] = *reinterpret_cast<const float4*>(p.bias + colg);
            cv[2 + jj] = *reinterpret_cast<const float4*>(p.bias + colg + 32);
            cv[4 + jj] = *reinterpret_cast<const float4*>(p.mean + ch);
            cv[6 + jj] = *reinterpret_cast<const float4*>(p.stdv + ch);
        }
    } else if constexpr (EPI != EPI_PARTIAL) {
#pragma unroll
        for (int j = 0; j < 4; ++j) cv[j] = *reinterpret_cast<const float4*>(p.bias + n0 + wn * 64 + j * 16 + 4 * cg);
    }
}

// K-split ping-pong launches (few tiles: a workgroup owns one K range of a tile): the raw accumulators of range `ks`
// go to partial[ks][B, Hout, Wout, N] with 16-byte stores; splitk_epilogue_kernel sums the ranges in a fixed order and
// applies the layer's epilogue.
__device__ __forceinline__ void halo16_epilogue_partial(const ConvParams& p, f32x4 (&acc)[4][4], int wm, int wn, int lane,
                                                        int n0, int tx0, int ty0, int b0, int ks) {
    const int px = lane & 15, cg = lane >> 4;
    const int x = tx0 + px, y0 = ty0 + wm * 4;
    float* const pbase = p.partial + (size_t)ks * ((size_t)p.B * p.Hout * p.Wout * p.N) +
                         ((size_t)b0 * p.Hout * p.Wout + x) * p.N + n0 + wn * 64 + 4 * cg;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<float4*>(pbase + (size_t)(y0 + i) * p.Wout * p.N + j * 16) = f4(acc[i][j]);
}

template <int EPI, bool SPLIT, bool OUT8 = false, bool OUTC = false>
__device__ __forceinline__ void halo16_epilogue_body(const ConvParams& p, f32x4 (&acc)[4][4], int wm, int wn, int lane,
                                                     int n0, int tx0, int ty0, int b0, int stat_tile,
                                                     float4 (&xin)[4][2], float4 (&cv)[8]) {
    const int px = lane & 15, cg = lane >> 4;
    const int x = tx0 + px, y0 = ty0 + wm * 4;
    float* const obase = p.out + (size_t)p.out_off + (size_t)b0 * p.out_pb + x * p.out_px;
    if constexpr (EPI == EPI_SPADE) {
        // columns come as (32 gamma | 32 beta) per 64: sub-tiles 0, 1 are gamma of channels ch0 + {0..15, 16..31},
        // sub-tiles 2, 3 their beta twins
        const int ch0 = (n0 + wn * 64) >> 1;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const float gq[4] = {cv[jj].x, cv[jj].y, cv[jj].z, cv[jj].w};
            const float bq[4] = {cv[2 + jj].x, cv[2 + jj].y, cv[2 + jj].z, cv[2 + jj].w};
            const float mq[4] = {cv[4 + jj].x, cv[4 + jj].y, cv[4 + jj].z, cv[4 + jj].w};
            float sq[4] = {cv[6 + jj].x, cv[6 + jj].y, cv[6 + jj].z, cv[6 + jj].w};
            if constexpr (SPLIT) {
#pragma unroll
                for (int k = 0; k < 4; ++k) sq[k] = 1.f / sq[k];          // bf16x3: multiply by 1/sigma
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float* orow = obase + (y0 + i) * p.out_py;
                const float xq[4] = {xin[i][jj].x, xin[i][jj].y, xin[i][jj].z, xin[i][jj].w};
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float normalized = SPLIT ? (xq[k] - mq[k]) * sq[k] : (xq[k] - mq[k]) / sq[k];
                    const float t = (acc[i][jj][k] + gq[k]) * normalized + (acc[i][jj + 2][k] + bq[k]);
                    v[k] = t >= 0.f ? t : t * p.slope;
                }
                if constexpr (OUTC) {
                    msr_store_f16c4_dev(orow, ch0 + jj * 16 + 4 * cg, v[0], v[1], v[2], v[3]);   // PREC_F16C consumer
                } else if constexpr (OUT8) {
                    // bf8 e5m2 bytes for a PREC_FP8 consumer: 4 consecutive channels = one dword
                    unsigned w8 = 0;
                    w8 = __builtin_amdgcn_cvt_pk_bf8_f32(v[0], v[1], w8, false);
                    w8 = __builtin_amdgcn_cvt_pk_bf8_f32(v[2], v[3], w8, true);
                    reinterpret_cast<unsigned*>(orow)[(ch0 + jj * 16 + 4 * cg) >> 2] = w8;
                } else if constexpr (SPLIT) {
                    // chunk image of the pixel: 16 words of hi pairs, 16 words of lo pairs
                    unsigned h01, l01, h23, l23;
                    msr_split_bf16_pk(v[0], v[1], h01, l01);
                    msr_split_bf16_pk(v[2], v[3], h23, l23);
                    unsigned* chunk = reinterpret_cast<unsigned*>(orow) + ch0 + jj * 8 + 2 * cg;
                    *reinterpret_cast<uint2*>(chunk) = make_uint2(h01, h23);
                    *reinterpret_cast<uint2*>(chunk + 16) = make_uint2(l01, l23);
                } else {
                    *reinterpret_cast<float4*>(orow + ch0 + jj * 16 + 4 * cg) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
    } else {
        // Fused output moments: sums of d = v - bias (a per-channel constant shift, the same in every lane, so the
        // 16 lanes of a column group add up directly) and d^2 over the 64 pixels of the wave.
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wn * 64 + j * 16 + 4 * cg;
            const float bq[4] = {cv[j].x, cv[j].y, cv[j].z, cv[j].w};
            float4 res[4];
            if constexpr (EPI == EPI_RES) {
                const float* abase = p.aux + (size_t)b0 * p.aux_pb + (x >> p.aux_shift) * p.aux_px + col;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    res[i] = *reinterpret_cast<const float4*>(abase + ((y0 + i) >> p.aux_shift) * p.aux_py);
            }
            // the lane's 4 values are shifted by its first one (a data value: offsets of the accumulator or of the residual
            // cancel, not only the bias); the 16 lanes of a row are combined as (mean, M2) with the between-lane term
            float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, pv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float d[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = acc[i][j][k];
                if constexpr (EPI == EPI_RES) { d[0] += res[i].x; d[1] += res[i].y; d[2] += res[i].z; d[3] += res[i].w; }
                *reinterpret_cast<float4*>(obase + (y0 + i) * p.out_py + col) =
                    make_float4(d[0] + bq[0], d[1] + bq[1], d[2] + bq[2], d[3] + bq[3]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (i == 0) pv[k] = d[k];
                    const float e = d[k] - pv[k];
                    s1[k] += e; s2[k] += e * e;
                }
            }
            if (p.stat_partial) {
                float mean[4], m2[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float mu = row16_sum(4.f * pv[k] + s1[k]) * (1.f / 64.f);
                    const float dl = (pv[k] - mu) + s1[k] * 0.25f;
                    const float t = row16_sum(s2[k] - s1[k] * s1[k] * 0.25f + 4.f * dl * dl);
                    mean[k] = bq[k] + mu;
                    m2[k] = t > 0.f ? t : 0.f;
                }
                if (px == 0) {
                    const int slab = stat_tile * 2 + wm;       // one slab per (8-row m-tile, wm): 64 pixels
                    float* o = p.stat_partial + (size_t)slab * 3 * p.N + col;
                    *reinterpret_cast<float4*>(o) = make_float4(64.f, 64.f, 64.f, 64.f);
                    *reinterpret_cast<float4*>(o + p.N) = make_float4(mean[0], mean[1], mean[2], mean[3]);
                    *reinterpret_cast<float4*>(o + 2 * p.N) = make_float4(m2[0], m2[1], m2[2], m2[3]);
                }
            }
        }
    }
}

// EPI_SPADE writing the f16c chunk image, assembled per pixel in LDS.  A lane's 4 channels are three pieces of the pixel's
// 128-byte chunk (8 bytes of fp16, 4 of h8, 4 of l8): stored straight from the lane that is SIX store instructions per tile
// row, each touching 16 lines with 4- or 8-byte pieces, and the epilogue is store-ISSUE-bound (tools/gpu_pp_stamps_gb.py: a
// gamma|beta tile takes 87.4k cycles, 79.4k with one 16-byte store per lane, 77.4k with none; MI355X_MICROARCH.md
// "epilogue store tail").  Here the wave writes the pieces of one tile row (16 pixels x 32 channels = 16 chunk lines) into
// a private 2.3 KB LDS image, reads each line back as two 16-byte quarters per lane and issues TWO stores per row, each
// 64 contiguous bytes per pixel.  Private to the wave (LDS operations of one wave execute in order): no barrier.
// F6 = true writes the PREC_F16C6 image (kernels.h): the block scale of a pixel's 32 channels needs the maximum over the four
// lanes that share the pixel (16 lanes apart) — they exchange it through the four pad dwords of the pixel's staged line — and
// the 6-bit codes of a lane's four channels are three bytes of the line, written as bytes.
template <bool F6>
__device__ __forceinline__ void halo16_epilogue_spade_f16c_staged(const ConvParams& p, f32x4 (&acc)[4][4], int wm, int wn,
                                                                  int lane, int n0, int tx0, int ty0, int b0,
                                                                  float4 (&xin)[4][2], float4 (&cv)[8], unsigned* stage) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    constexpr int SP = 36;                                     // dwords per staged line (32 + pad: spreads the pixels over banks)
    const int px = lane & 15, cg = lane >> 4;
    const int x = tx0 + px, y0 = ty0 + wm * 4;
    const int ch0 = (n0 + wn * 64) >> 1;                       // first of the wave's 32 output channels: one whole chunk
    float* const obase = p.out + (size_t)p.out_off + (size_t)b0 * p.out_pb + x * p.out_px + ch0;
    unsigned* const line = stage + px * SP;
    float rs[2][4];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        rs[jj][0] = 1.f / cv[6 + jj].x; rs[jj][1] = 1.f / cv[6 + jj].y; rs[jj][2] = 1.f / cv[6 + jj].z; rs[jj][3] = 1.f / cv[6 + jj].w;
    }
    if constexpr (F6) {     // the zero bytes behind the two scale bytes of a line (dwords 23 and 31) never change
        if (cg == 0) { line[23] = 0u; line[31] = 0u; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v[2][4];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const float gq[4] = {cv[jj].x, cv[jj].y, cv[jj].z, cv[jj].w};
            const float bq[4] = {cv[2 + jj].x, cv[2 + jj].y, cv[2 + jj].z, cv[2 + jj].w};
            const float mq[4] = {cv[4 + jj].x, cv[4 + jj].y, cv[4 + jj].z, cv[4 + jj].w};
            const float xq[4] = {xin[i][jj].x, xin[i][jj].y, xin[i][jj].z, xin[i][jj].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float normalized = (xq[k] - mq[k]) * rs[jj][k];
                const float t = (acc[i][jj][k] + gq[k]) * normalized + (acc[i][jj + 2][k] + bq[k]);
                float u = t >= 0.f ? t : t * p.slope;
                v[jj][k] = u > 65504.f ? 65504.f : (u < -65504.f ? -65504.f : u);           // as msr_store_f16c4_dev
            }
        }
        float inv = 1.f;        // F6: 2^-E of the pixel's block scale
        if constexpr (F6) {
            float m = 0.f;
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int k = 0; k < 4; ++k) m = fmaxf(m, fabsf(v[jj][k]));       // NaN: dropped here, kept in the fp16 piece
            line[32 + cg] = __builtin_bit_cast(unsigned, m);
            asm volatile("" ::: "memory");
            const uint4 mm = *reinterpret_cast<const uint4*>(line + 32);
            asm volatile("" ::: "memory");
            const float amax = fmaxf(fmaxf(__builtin_bit_cast(float, mm.x), __builtin_bit_cast(float, mm.y)),
                                     fmaxf(__builtin_bit_cast(float, mm.z), __builtin_bit_cast(float, mm.w)));
            const int eb = msr_block_e8m0_dev(amax);
            inv = __builtin_bit_cast(float, (254 - eb) << 23);                   // 2^-(eb - 127)
            if (cg == 0) line[22] = (unsigned)eb;                                // byte 88: the h6 piece's e8m0
            if (cg == 1) line[30] = (unsigned)(eb - 11);                         // byte 120: the l6 piece's
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const h2 a = {(_Float16)v[jj][0], (_Float16)v[jj][1]}, b = {(_Float16)v[jj][2], (_Float16)v[jj][3]};
            const float l0 = (v[jj][0] - (float)a[0]) * 2048.f, l1 = (v[jj][1] - (float)a[1]) * 2048.f;
            const float l2 = (v[jj][2] - (float)b[0]) * 2048.f, l3 = (v[jj][3] - (float)b[1]) * 2048.f;
            // the chunk image of the pixel: dwords 0..15 fp16 pairs (channel 16 jj + 4 cg + {0..3})
            *reinterpret_cast<uint2*>(line + jj * 8 + 2 * cg) = make_uint2(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b));
            if constexpr (F6) {
                // 4 codes = 24 bits = bytes 64 + 3 * (4 jj + cg) .. of the line (l6: 96 + ...)
                const unsigned h6 = msr_pack_e2m3x4_dev(v[jj][0] * inv, v[jj][1] * inv, v[jj][2] * inv, v[jj][3] * inv);
                const unsigned l6 = msr_pack_e2m3x4_dev(l0 * inv, l1 * inv, l2 * inv, l3 * inv);
                unsigned char* lb = reinterpret_cast<unsigned char*>(line) + 3 * (4 * jj + cg);
                lb[64] = (unsigned char)h6; lb[65] = (unsigned char)(h6 >> 8); lb[66] = (unsigned char)(h6 >> 16);
                lb[96] = (unsigned char)l6; lb[97] = (unsigned char)(l6 >> 8); lb[98] = (unsigned char)(l6 >> 16);
            } else {
                unsigned h8 = 0, l8 = 0;
                h8 = __builtin_amdgcn_cvt_pk_fp8_f32(v[jj][0], v[jj][1], h8, false);
                h8 = __builtin_amdgcn_cvt_pk_fp8_f32(v[jj][2], v[jj][3], h8, true);
                l8 = __builtin_amdgcn_cvt_pk_fp8_f32(l0, l1, l8, false);
                l8 = __builtin_amdgcn_cvt_pk_fp8_f32(l2, l3, l8, true);
                line[16 + jj * 4 + cg] = h8;                   // dwords 16..23 h8, 24..31 l8
                line[24 + jj * 4 + cg] = l8;
            }
        }
        // quarter cg of each half of the line (compiler barriers: the pieces were written through other types)
        asm volatile("" ::: "memory");
        const uint4 q0 = *reinterpret_cast<const uint4*>(line + 4 * cg);
        const uint4 q1 = *reinterpret_cast<const uint4*>(line + 16 + 4 * cg);
        asm volatile("" ::: "memory");
        unsigned* orow = reinterpret_cast<unsigned*>(obase + (y0 + i) * p.out_py);
        *reinterpret_cast<uint4*>(orow + 4 * cg) = q0;
        *reinterpret_cast<uint4*>(orow + 16 + 4 * cg) = q1;
    }
}

template <int EPI>
__device__ __forceinline__ void halo16_epilogue(const ConvParams& p, const TileGeom& g, f32x4 (&acc)[4][4], int wm, int wn,
                                                int lane, int n0, int tx0, int ty0, int b0, float4 (&xin)[4][2],
                                                float4 (&cv)[8], unsigned* stage = nullptr) {
    const int stat_tile = (b0 * g.tiles_y + (ty0 >> g.th_l)) * g.tiles_x + (tx0 >> g.tw_l);
    // a narrow output image (fp16 / fp8 / bf8 pieces): the conversions saturate, and only they run with the bit set
    const bool narrow = EPI == EPI_SPADE && p.out_split > OUT_BF16X3;
    if (narrow) msr_saturate_begin(acc);
    if constexpr (EPI == EPI_SPADE) {
        if (p.out_split == OUT_F16C6 && stage) halo16_epilogue_spade_f16c_staged<true>(p, acc, wm, wn, lane, n0, tx0, ty0, b0, xin, cv, stage);
        else if (p.out_split == OUT_F16C && stage) halo16_epilogue_spade_f16c_staged<false>(p, acc, wm, wn, lane, n0, tx0, ty0, b0, xin, cv, stage);
        else if (p.out_split == OUT_F16C) halo16_epilogue_body<EPI, true, false, true>(p, acc, wm, wn, lane, n0, tx0, ty0, b0, stat_tile, xin, cv);
        else if (p.out_split == OUT_BF8) halo16_epilogue_body<EPI, true, true>(p, acc, wm, wn, lane, n0, tx0, ty0, b0, stat_tile, xin, cv);
        else if (p.out_split) halo16_epilogue_body<EPI, true>(p, acc, wm, wn, lane, n0, tx0, ty0, b0, stat_tile, xin, cv);
        else halo16_epilogue_body<EPI, false>(p, acc, wm, wn, lane, n0, tx0, ty0, b0, stat_tile, xin, cv);
    } else {
        halo16_epilogue_body<EPI, false>(p, acc, wm, wn, lane, n0, tx0, ty0, b0, stat_tile, xin, cv);
    }
    if (narrow) msr_saturate_end();
}

}  // namespace msr

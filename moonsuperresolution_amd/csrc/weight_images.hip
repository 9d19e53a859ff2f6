// weight_images.hip — the weight images of the conv kernels: pure functions from host arrays to host arrays (no handle, no
// HIP call; upload_conv_weight in api.hip puts them on the device).  The image bits depend on clang's _Float16 conversions
// and on no contraction: this unit is compiled with hipcc and the library's flags (-ffp-contract=off).
#include "host.h"

namespace msr {

// HWIO [kh,kw,Cin,Cout] -> [tap][Cout][Cin]  (K contiguous per output channel, the igemm B-operand layout)
void hwio_to_tap_oc_ic(const float* src, float* dst, int taps, int cin, int cout, int dst_rows, const int* rowmap) {
    for (int t = 0; t < taps; ++t)
        for (int ci = 0; ci < cin; ++ci) {
            const float* s = src + ((size_t)t * cin + ci) * cout;
            for (int co = 0; co < cout; ++co) {
                const int row = rowmap ? rowmap[co] : co;
                dst[((size_t)t * dst_rows + row) * cin + ci] = s[co];
            }
        }
}

// The split images IMG_BF16, IMG_BF16_FRAG and IMG_F16 of [taps][N][Cin] weights.  Weights consumed by conv_igemm_bf16x3
// are uploaded in MFMA-fragment order (conv_igemm.hip):
//   [tap][chunk of 32 k][n-tile of 32][kg][hi|lo][lane = 32*h + j][8 bf16],  value = W[tap][32*nt + j][32*cc + 16*kg + 8*h + e]
// N and Cin are multiples of 32.
std::vector<float> build_split_image(const float* host, int taps, int N, int Cin, WeightImage img) {
    const size_t floats = (size_t)taps * N * Cin;
    std::vector<float> t(floats);
    if (img == IMG_F16) {
        // split-fp16 image of [tap][N][Cin] (PREC_F16X2 reads only the hi half of every chunk)
        for (size_t i = 0; i + 3 < floats; i += 4)
            msr_store_split4_f16(t.data() + (i & ~(size_t)31), (int)(i & 31), host[i], host[i + 1], host[i + 2], host[i + 3]);
        return t;
    }
    if (img == IMG_BF16) {
        // split-bf16 image of [tap][N][Cin]: every 32 consecutive k become [32 hi | 32 lo]
        for (size_t i = 0; i + 3 < floats; i += 4)
            msr_store_split4(t.data() + (i & ~(size_t)31), (int)(i & 31), host[i], host[i + 1], host[i + 2], host[i + 3]);
        return t;
    }
    uint16_t* o = reinterpret_cast<uint16_t*>(t.data());
    const int chunks = Cin / 32, nt32 = N / 32;
    for (int tap = 0; tap < taps; ++tap)
        for (int cc = 0; cc < chunks; ++cc)
            for (int nt = 0; nt < nt32; ++nt) {
                uint16_t* blk = o + (((size_t)tap * chunks + cc) * nt32 + nt) * 2048;   // 1024 floats
                for (int kg = 0; kg < 2; ++kg)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int j = lane & 31, hh = lane >> 5;
                        const float* src = host + ((size_t)tap * N + nt * 32 + j) * Cin + cc * 32 + kg * 16 + hh * 8;
                        uint16_t* hi = blk + ((kg * 2 + 0) * 64 + lane) * 8;
                        uint16_t* lo = blk + ((kg * 2 + 1) * 64 + lane) * 8;
                        for (int e = 0; e < 8; ++e) {
                            unsigned a, b2;
                            msr_split_bf16(src[e], a, b2);
                            hi[e] = (uint16_t)a; lo[e] = (uint16_t)b2;
                        }
                    }
            }
    return t;
}

// Effective per-parity taps of the head kernel, weff[py][px][dy + 1][dx + 1][C] (zero where a tap does not exist):
//  * Conv2D(1, 4, 'same') applied to a nearest-2x up-sampled tensor (networks.py:54-56), kernel HWIO [4,4,C,1]: TF SAME for
//    k = 4 pads 1 before / 2 after; output parity p reads up-sampled rows 2y + p - 1 + kh, i.e. half-resolution offsets
//    {-1, 0, 0, +1} (p = 0) or {0, 0, +1, +1} (p = 1) for kh = 0..3 — taps that land on the same pixel are summed;
//  * Conv2DTranspose(1, 4, strides 2, 'same') (pix2pix.py:53-57), kernel [4,4,1,C]: four stride-1 2 x 2 convolutions, one per
//    output parity: out[2y + py][2x + px] = sum_{t,u} in[y - 1 + py + t][x - 1 + px + u] * W[kmap(py,t)][kmap(px,u)],
//    kmap(0, .) = {3, 1}, kmap(1, .) = {2, 0}.
std::vector<float> head_weff_upconv(const float* k44c, int C) {
    std::vector<float> weff((size_t)36 * C, 0.f);
    auto dmap = [](int parity, int k) { return parity == 0 ? (k == 0 ? 0 : k == 3 ? 2 : 1) : (k < 2 ? 1 : 2); };
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px)
            for (int kh = 0; kh < 4; ++kh)
                for (int kw = 0; kw < 4; ++kw) {
                    float* dst = &weff[((((size_t)py * 2 + px) * 3 + dmap(py, kh)) * 3 + dmap(px, kw)) * C];
                    const float* src = k44c + ((size_t)kh * 4 + kw) * C;
                    for (int c = 0; c < C; ++c) dst[c] += src[c];
                }
    return weff;
}
// The head's effective taps as A operands of v_mfma_f32_16x16x32_f16 for the head epilogue of conv_igemm_f16c_sw (conv_sw.hip
// sw_epilogue_head), C = 128: [wave 4][slot block 2][hi | lo][lane 64] x 8 fp16 = 16 KB.  Lane (s = lane & 15, cg = lane >> 4)
// holds slot 16 sb + s (kernels.h HEAD_SLOTS, zero from slot 25 on) at the lane's 8 K positions, K position e = channel
// 64 (wave >> 1) + 16 (wave & 1) + 32 (e >> 2) + 4 cg + (e & 3): the order in which the wave's accumulators hold a pixel.
std::vector<float> build_head_wfrag(const float* k44c) {
    constexpr int C = 128;
    const std::vector<float> weff = head_weff_upconv(k44c, C);
    std::vector<float> img(4096, 0.f);
    uint16_t* const t = reinterpret_cast<uint16_t*>(img.data());
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px)
            for (int dy = py; dy < 3; ++dy)
                for (int dx = px; dx < 3; ++dx) {
                    const int slot = head_slot(py, px, dy, dx), sb = slot >> 4, s = slot & 15;
                    const float* src = &weff[((((size_t)py * 2 + px) * 3 + dy) * 3 + dx) * C];
                    for (int w = 0; w < 4; ++w)
                        for (int cg = 0; cg < 4; ++cg)
                            for (int e = 0; e < 8; ++e) {
                                const int c = 64 * (w >> 1) + 16 * (w & 1) + 32 * (e >> 2) + 4 * cg + (e & 3);
                                unsigned hi, lo;
                                msr_split_f16(src[c], hi, lo);
                                const int lane = 16 * cg + s;
                                t[(((w * 2 + sb) * 2 + 0) * 64 + lane) * 8 + e] = (uint16_t)hi;
                                t[(((w * 2 + sb) * 2 + 1) * 64 + lane) * 8 + e] = (uint16_t)lo;
                            }
                }
    return img;
}
std::vector<float> head_weff_transpose(const float* k44c, int C) {
    static const int kmap[2][2] = {{3, 1}, {2, 0}};
    std::vector<float> weff((size_t)36 * C, 0.f);
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px)
            for (int t = 0; t < 2; ++t)
                for (int u = 0; u < 2; ++u) {
                    const float* src = k44c + ((size_t)kmap[py][t] * 4 + kmap[px][u]) * C;
                    std::copy(src, src + C, &weff[((((size_t)py * 2 + px) * 3 + (py + t)) * 3 + (px + u)) * C]);
                }
    return weff;
}

// channels of an fp8 tensor: 128 (one chunk: the two-tiles-per-body form of the kernel) or a multiple of 256 (chunk pairs)
int fp8_pad(int cin) { return cin <= 128 ? 128 : (cin + 255) / 256 * 256; }

// position e of a 32-channel chunk holds channel GBR_PERM(e): the order in which phase 1 of conv_gb_resident leaves a pixel's
// channels in a lane (32 x 32 MFMA rows 8q + 4h + r, halves interleaved by v_cvt_scalef32_2xpk16_fp6_f32)
static inline int gbr_perm(int e) { return 8 * (e >> 3) + 4 * (e & 1) + ((e >> 1) & 3); }

// f16c6 image of [taps][N][Cin] weights (kernels.h PREC_F16C6): per 32-channel chunk [32 x hi f16 | 24 B l6 | e8m0 | 0.. |
// 24 B h6 | e8m0 | 0..], one power-of-two scale per output channel and piece (2^E >= max / 7.5)
std::vector<float> build_f16c6_image(const float* host, int taps, int N, int Cin) {
    std::vector<float> img((size_t)taps * N * Cin, 0.f);
    auto pow2exp = [](float amax) {       // NOT pow2exp_e4m3: the divisor, the double arithmetic and the m == 0.5 step differ
        if (!(amax > 0.f)) return 0;
        int fe;
        // in double: amax / 7.5f rounded to float can land ON a power of two from just above it, and 2^E would then be
        // smaller than amax / 7.5 (kernels.h PREC_F16C6: 2^E >= max / 7.5)
        const double m = std::frexp((double)amax / 7.5, &fe);       // amax / 7.5 = m * 2^fe, m in [0.5, 1)
        return std::max(-100, std::min(100, m == 0.5 ? fe - 1 : fe));
    };
    for (int n = 0; n < N; ++n) {
        float ah = 0.f, al = 0.f;
        for (int t = 0; t < taps; ++t)
            for (int k = 0; k < Cin; ++k) {
                const float w = host[((size_t)t * N + n) * Cin + k];
                const float hi = (float)(_Float16)w;
                ah = std::max(ah, std::fabs(w));
                al = std::max(al, std::fabs(w - hi));
            }
        const int eh = pow2exp(ah), el = pow2exp(al);
        const float ih = std::ldexp(1.f, -eh), il = std::ldexp(1.f, -el);
        for (int t = 0; t < taps; ++t)
            for (int c0 = 0; c0 < Cin; c0 += 32) {
                unsigned char* chunk = reinterpret_cast<unsigned char*>(img.data() + ((size_t)t * N + n) * Cin + c0);
                unsigned long long bl[3] = {0, 0, 0}, bh[3] = {0, 0, 0};      // 192-bit little-endian strings
                for (int c = 0; c < 32; ++c) {
                    const float w = host[((size_t)t * N + n) * Cin + c0 + c];
                    const _Float16 hi = (_Float16)w;
                    reinterpret_cast<_Float16*>(chunk)[c] = hi;
                    const unsigned long long cl = msr_f32_to_e2m3((w - (float)hi) * il), ch = msr_f32_to_e2m3(w * ih);
                    const int pos = 6 * c;
                    bl[pos / 64] |= cl << (pos % 64);
                    if (pos % 64 > 58) bl[pos / 64 + 1] |= cl >> (64 - pos % 64);
                    bh[pos / 64] |= ch << (pos % 64);
                    if (pos % 64 > 58) bh[pos / 64 + 1] |= ch >> (64 - pos % 64);
                }
                std::memcpy(chunk + 64, bl, 24);
                chunk[88] = (unsigned char)(127 + el);
                std::memcpy(chunk + 96, bh, 24);
                chunk[120] = (unsigned char)(127 + eh);
            }
    }
    return img;
}

// The weight stream of conv_gb_resident (conv_gbr.hip): the f16c6 image of [9][N][128] (input channels of every 32-chunk in
// the kernel's position order, gbr_perm) re-ordered into the order the kernel's waves load it — for channel block nt, wave q,
// tap pair P (K-steps 2P, 2P + 1 of the 36-step chunk-major sequence: step T = chunk T / 9, tap T % 9), column block j, piece
// (0 / 1: fp16 fragment of the even / odd step, 2 / 3: first / second 16 bytes of the lane's fp6 piece), lane: 16 bytes.
// Lane (px, cg): row = 128 nt + 64 (q >> 1) + 16 (q & 1) + 32 j + px; fp16 fragment = bytes 16 cg .. of the record; fp6 piece =
// bytes 64 + 32 (cg & 1) .. of the even step's record (cg < 2) or the odd step's (cg >= 2).
std::vector<float> gbr_weight_stream(const float* w_tap_n_k, int N) {
    const int Cin = 128;
    std::vector<float> perm((size_t)9 * N * Cin);
    for (size_t row = 0; row < (size_t)9 * N; ++row)
        for (int k = 0; k < Cin; ++k) perm[row * Cin + k] = w_tap_n_k[row * Cin + (k & ~31) + gbr_perm(k & 31)];
    const std::vector<float> img = build_f16c6_image(perm.data(), 9, N, Cin);
    const unsigned char* src = reinterpret_cast<const unsigned char*>(img.data());
    std::vector<float> out(img.size());
    unsigned char* dst = reinterpret_cast<unsigned char*>(out.data());
    auto rec = [&](int T, int row) { return src + (((size_t)(T % 9) * N + row) * 4 + T / 9) * 128; };
    for (int nt = 0; nt < N / 128; ++nt)
        for (int q = 0; q < 4; ++q)
            for (int P = 0; P < 18; ++P)
                for (int j = 0; j < 2; ++j)
                    for (int piece = 0; piece < 4; ++piece)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int px = lane & 15, cg = lane >> 4;
                            const int row = 128 * nt + 64 * (q >> 1) + 16 * (q & 1) + 32 * j + px;
                            const unsigned char* s;
                            if (piece < 2) s = rec(2 * P + piece, row) + 16 * cg;
                            else s = rec(2 * P + (cg >> 1), row) + 64 + 32 * (cg & 1) + 16 * (piece - 2);
                            std::memcpy(dst + ((((((size_t)nt * 4 + q) * 18 + P) * 2 + j) * 4 + piece) * 64 + lane) * 16, s, 16);
                        }
    return out;
}

// Exponent of the power-of-two scale of the e4m3 pieces (f16c, fp8): amax / 448 = m * 2^fe with m in [0.5, 1), so 2^fe >=
// amax / 448 and the largest |w| of the channel lands in e4m3's top binade.  Clamped to +-100; 0 for an all-zero channel.
static int pow2exp_e4m3(float amax) {
    if (!(amax > 0.f)) return 0;
    int fe;
    (void)std::frexp(amax / 448.f, &fe);
    return std::max(-100, std::min(100, fe));
}

// f16c image of [taps][N][Cin] weights (kernels.h PREC_F16C): per 32-channel chunk [32 x hi f16 | 32 x l8 | 32 x h8]
// with hi = f16_rn(w), l8 = e4m3((w - hi) * 2^-el), h8 = e4m3(w * 2^-eh), el / eh powers of two
// per output channel; wexp[n] = (127 + el) | (127 + eh) << 8 (uploaded as key + ".wexp").  Cin is a multiple of 32.
std::vector<float> build_f16c_image(const float* host, int taps, int N, int Cin, std::vector<int>& wexp) {
    std::vector<float> img((size_t)taps * N * Cin);
    wexp.assign(N, 0);
    for (int n = 0; n < N; ++n) {
        float ah = 0.f, al = 0.f;
        for (int t = 0; t < taps; ++t)
            for (int k = 0; k < Cin; ++k) {
                const float w = host[((size_t)t * N + n) * Cin + k];
                const float hi = (float)(_Float16)w;
                ah = std::max(ah, std::fabs(w));
                al = std::max(al, std::fabs(w - hi));
            }
        const int eh = pow2exp_e4m3(ah), el = pow2exp_e4m3(al);
        const float ih = std::ldexp(1.f, -eh), il = std::ldexp(1.f, -el);
        wexp[n] = (127 + el) | ((127 + eh) << 8);
        for (int t = 0; t < taps; ++t)
            for (int c0 = 0; c0 < Cin; c0 += 32) {
                unsigned char* chunk = reinterpret_cast<unsigned char*>(img.data() + ((size_t)t * N + n) * Cin + c0);
                for (int c = 0; c < 32; ++c) {
                    const float w = host[((size_t)t * N + n) * Cin + c0 + c];
                    const _Float16 hi = (_Float16)w;
                    reinterpret_cast<_Float16*>(chunk)[c] = hi;
                    chunk[64 + c] = msr_f32_to_e4m3((w - (float)hi) * il);
                    chunk[96 + c] = msr_f32_to_e4m3(w * ih);
                }
            }
    }
    return img;
}

// fp8 e4m3 image of [taps][N][Cin] weights: bytes [taps][N][fp8_pad(Cin)] (zero padded), a power-of-two scale per output
// channel, its e8m0 exponent replicated in the four bytes of wexp[n] (uploaded as key + ".wexp")
std::vector<float> build_fp8_image(const float* host, int taps, int N, int Cin, std::vector<int>& wexp) {
    const int cp = fp8_pad(Cin);
    std::vector<float> img((size_t)taps * N * cp / 4, 0.f);
    unsigned char* q = reinterpret_cast<unsigned char*>(img.data());
    wexp.assign(N, 0);
    for (int n = 0; n < N; ++n) {
        float amax = 0.f;
        for (int t = 0; t < taps; ++t)
            for (int k = 0; k < Cin; ++k) amax = std::max(amax, std::fabs(host[((size_t)t * N + n) * Cin + k]));
        const int e = pow2exp_e4m3(amax);
        const float inv = std::ldexp(1.f, -e);
        for (int t = 0; t < taps; ++t)
            for (int k = 0; k < Cin; ++k)
                q[((size_t)t * N + n) * cp + k] = msr_f32_to_e4m3(host[((size_t)t * N + n) * Cin + k] * inv);
        const unsigned b = (unsigned)(127 + e);
        wexp[n] = (int)(b | (b << 8) | (b << 16) | (b << 24));
    }
    return img;
}

}  // namespace msr

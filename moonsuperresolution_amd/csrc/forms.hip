// forms.hip — the form table: which kernel runs every conv layer of the generator and which weight image that kernel reads
// (conv_form, spade_form, pp_ksplit), fixed by the handle's batch, size and flags.  msr_load_weight and the planner both read
// it, so a layer's weights are always in the layout its launch expects.
#include "host.h"

namespace msr {

// K split of the persistent ping-pong kernel for layers with fewer 16 x 16 x 128 tiles than CUs: whole chunk pairs
// per range, a power of two, as many ranges as it takes to give every CU a work item.  0 = the layer is not one for
// that kernel (it needs stride 1, r >= 16, Cin % 64 == 0, an input below the 2 GiB buffer-descriptor range and, split
// or not, at least `min_items` work items — below that the small-tile split-K kernels are faster).
static int pp_ksplit(int B, int rout, int N, int stride, int cin, long min_items = 128) {
    static const bool off = env_int("MSR_PP_KSPLIT", 1) == 0;
    if (stride != 1 || rout < 16 || cin % 64 || N % 128) return 0;
    if ((size_t)B * (rout + 2) * (rout + 2) * cin * sizeof(float) >= ((size_t)1 << 31)) return 0;
    const long tiles = (long)B * (rout / 16) * (rout / 16) * (N / 128);
    if (tiles >= 256) return 1;
    if (off) return 0;
    const int pairs = cin / 64;
    int ks = 1;
    while (tiles * ks * 2 <= 256 && pairs % (ks * 2) == 0) ks *= 2;
    return tiles * ks >= min_items ? ks : 0;
}

// A conv form; its weight image follows from the precision (and, under bf16x3, from the fragment order).
ConvForm make_form(int prec, int tile, int ksplit, int wt_frag, int no_cross) {
    ConvForm f;
    f.prec = prec; f.tile = tile; f.ksplit = ksplit; f.wt_frag = wt_frag; f.no_cross = no_cross;
    switch (prec) {
        case PREC_BF16X3: f.img = wt_frag ? IMG_BF16_FRAG : IMG_BF16; break;
        case PREC_F16X2: f.img = IMG_F16; break;
        case PREC_FP8: f.img = IMG_FP8; break;
        case PREC_F16C: f.img = IMG_F16C; break;
        case PREC_F16C6: f.img = IMG_F16C6; break;
        default: f.img = IMG_F32;
    }
    return f;
}

// Form of a plain conv in `prec` (PREC_F32 or PREC_BF16X3): the encoder's stride-2 convs, the pix2pix convs, the kernel-level
// entries and every generator conv that no quantised form covers.  The tile and the K split follow the shape
// (conv_pick_tile / conv_pick_ksplit, conv_igemm.hip); under bf16x3 the persistent ping-pong kernel takes the layers that
// pp_ksplit accepts.
ConvForm conv_form(int B, int rout, int N, int stride, int epi, int prec, int cin, int taps) {
    const int M = B * rout * rout, ksteps = taps * (cin / 32);
    int tile = conv_pick_tile(M, N, epi, prec, ksteps), wt_frag = 0, ksplit = 0;   // ksplit 0: conv_pick_ksplit decides
    if (prec == PREC_BF16X3) {
        const long big_blocks = (long)((M + 127) / 128) * (N / 128);
        const int pks = pp_ksplit(B, rout, N, stride, cin);
        if (pks >= 1) {
            // LDS-staged input halo, 512-thread ping-pong form (one persistent workgroup per CU, 16 x 16 pixels x 128
            // channels per tile): 10-25 % faster than two 256-thread workgroups per CU as soon as it fills the chip
            // once; with fewer tiles than CUs, K ranges supply the work items (pks > 1).
            tile = TILE_256x128_PP;
            ksplit = pks;
        } else if (tile == TILE_64x64 || big_blocks < 256) {
            wt_frag = 1;   // few workgroups (with split-K): B fragments straight to VGPRs, +18 % on the small tile
        } else if (stride == 1 && rout >= 16 && cin % 64 == 0 &&
                   (size_t)B * (rout + 2) * (rout + 2) * cin * sizeof(float) < ((size_t)1 << 31)) {   // raw buffer loads: 2 GiB
            tile = TILE_128x128_HALO16;     // only reached with MSR_PP_KSPLIT=0: two 256-thread workgroups per CU
            ksplit = 1;
        }
    }
    return make_form(prec, tile, ksplit > 0 ? ksplit : conv_pick_ksplit(M, N, ksteps, tile, prec), wt_frag);
}

// out_split of a producer whose output feeds a conv in `prec`: the operand image that conv reads
static int split_for(int prec) {
    switch (prec) {
        case PREC_BF16X3: return OUT_BF16X3;
        case PREC_F16X2: return OUT_F16X2;
        case PREC_FP8: return OUT_BF8;
        case PREC_F16C: return OUT_F16C;
        case PREC_F16C6: return OUT_F16C6;
        default: return OUT_F32;
    }
}

// Form of the SPADE layer that normalises C channels at resolution r, and of the conv C -> cout (epilogue epi) it feeds.
// Under the quantised modes a conv takes the quantised form when it runs the persistent ping-pong kernel, and a consumer
// only when its gamma|beta conv does too: that conv's epilogue writes the consumer's operand image.  Every other conv runs
// the plain form of the handle's precision.
//  * MSR_FLAG_FP8: a conv whose whole tiles fill the chip (B * (r/16)^2 * (N/128) >= 256, no K split).  Its input holds one
//    byte per channel: 128 channels (one 128-byte chunk) or a multiple of 256 (chunk pairs), in float slots of 4 channels.
//  * MSR_FLAG_F16C: the same rule, with the K-range launches of the ping-pong kernel (fewer tiles than CUs) taken too: their
//    split-K epilogue writes the f16c image (MSR_F16C_KSPLIT=0: whole-tile launches only).
//  * PREC_F16C6 (fp6 cross terms, kernels.h), OPT-IN with MSR_F16C_FP6=1: the f16c consumers that run the stream kernel
//    (conv_sw.hip: whole tiles, Cin % 128 == 0) behind a whole-tile gamma|beta conv (its LDS-assembled epilogue writes the
//    fp6 image).  Measured: the consumer gains 6.5 % on those convs, the producer's block-scale and 6-bit packing
//    cost the gamma|beta epilogues more, net -1 % per call: it pays only once the gamma|beta convs consume fp6 too.  Any
//    MSR_F16C_SW other than 1 (the A/B dispatches) switches it off.
//  * conv_gb_resident (conv_gbr.hip) takes a layer whose gamma|beta conv and f16c consumer run f16c, when the
//    layer has enough 16 x 16 pixel tiles x channel-block ranges to fill the chip (conv_gbr_ranges; MSR_GBR=0 switches it
//    off).  Its weights are the f16c6 image with the input channels of every 32-chunk in the kernel's order (gbr_perm).
//    Under the environment switch it leaves the f16c6 consumers to the ping-pong kernel (the measured -1 % above).
//  * MSR_FLAG_CROSS_FP6: the same f16c6 consumers as MSR_F16C_FP6=1 selects, and their layers KEEP conv_gb_resident, which
//    then writes the fp6 image (OUT_F16C6); where it does not take the layer the ping-pong epilogue writes it as above.
//  * MSR_FLAG_GB_F16X2: a gamma|beta conv that runs the ping-pong kernel on whole tiles takes 2-term fp16 products (the
//    K-split launches run the 3-term form).
static SpadeForm spade_form(const msr_handle* h, int r, int C, int cout, int epi) {
    static const bool f16c_ks_off = env_int("MSR_F16C_KSPLIT", 1) == 0;
    static const bool fp6_on = env_int("MSR_F16C_FP6", 0) == 1 && env_int("MSR_F16C_SW", 1) == 1;
    const int B = h->B;
    auto fills = [&](int N) { return r >= 16 && N % 128 == 0 && (long)B * (r / 16) * (r / 16) * (N / 128) >= 256; };
    auto f16c_pp = [&](int N, int cin) { return f16c_ks_off ? fills(N) : pp_ksplit(B, r, N, 1, cin) >= 1; };
    const bool gb8 = h->fp8 && fills(2 * C), cv8 = gb8 && fills(cout);
    const bool gbc = h->f16c && f16c_pp(2 * C, 128), cvc = gbc && C % 64 == 0 && f16c_pp(cout, C);
    static const bool sw_on = env_int("MSR_F16C_SW", 1) == 1;      // the f16c6 consumer is the stream kernel
    const bool cv6 = cvc && (fp6_on || (h->cross6 && sw_on)) && C % 128 == 0 && fills(cout) && fills(2 * C);
    SpadeForm s;
    s.gbr = cvc && (!cv6 || h->cross6) && conv_gbr_ranges(B, r, 2 * C) > 0;
    if (gb8) {
        s.gb = make_form(PREC_FP8, TILE_256x128_PP, 1);
    } else if (s.gbr) {
        s.gb = make_form(PREC_F16C6, TILE_256x128_PP, 1, 0, h->f16m);
        s.gb.img = IMG_GBR;
    } else if (gbc) {
        s.gb = make_form(PREC_F16C, TILE_256x128_PP, pp_ksplit(B, r, 2 * C, 1, 128));   // > 1: K ranges
    } else {
        s.gb = conv_form(B, r, 2 * C, 1, EPI_SPADE, h->prec, 128);
        if (h->gb_f16x2 && s.gb.tile == TILE_256x128_PP && s.gb.ksplit == 1) s.gb = make_form(PREC_F16X2, TILE_256x128_PP, 1);
    }
    if (cv8) s.cv = make_form(PREC_FP8, TILE_256x128_PP, 1);
    else if (cv6) s.cv = make_form(PREC_F16C6, TILE_256x128_PP, 1);
    else if (cvc) {
        // the f16 mode leaves the cross terms out on the stream kernel (whole tiles) only: a K-range launch runs the
        // ping-pong kernel, which has no such form and computes them
        const int ks = pp_ksplit(B, r, cout, 1, C);
        s.cv = make_form(PREC_F16C, TILE_256x128_PP, ks, 0, h->f16m && ks == 1);
    }
    else s.cv = conv_form(B, r, cout, 1, epi, h->prec, C);
    s.h_split = split_for(s.gb.prec);
    s.hslots = gb8 ? fp8_pad(128) / 4 : 128;
    s.a_split = split_for(s.cv.prec);
    s.aslots = cv8 ? fp8_pad(C) / 4 : C;
    return s;
}

// The forms of the SPADE generator's convs, fixed by the handle's batch, size and flags: msr_load_weight builds every
// weight image from this table and plan_spade launches every layer by it.
void fill_forms(msr_handle* h) {
    if (h->variant == MSR_PIX2PIX) return;
    for (int i = 2; i <= 5; ++i)
        h->enc_forms[i] = conv_form(h->B, h->S >> i, kEncChannels[i - 1], 2, EPI_BIAS, h->prec, kEncChannels[i - 2]);
    int cin = 1024;
    for (int i = 1; i <= 6; ++i) {
        const int f = kGenFilters[i - 1], r = (h->S / 64) << (i - 1);
        for (int j = 1; j <= (f != cin ? 3 : 2); ++j)       // spade_2 normalises conv_1's output
            h->spade_forms[i][j] = spade_form(h, r, j == 2 ? f : cin, f, j == 2 ? EPI_RES : EPI_BIAS);
        cin = f;
    }
}

// The fused head (kernels.h EPI_RES_HEAD) is one instantiation of the stream kernel: gen.rb6.conv_2 (128 -> 128 at r = S / 2)
// takes it when it runs there on whole tiles in the plain f16c form.  Anywhere else (K ranges on the ping-pong kernel at small
// shapes, MSR_F16C_SW other than 1) the plan keeps the separate head: a fallback, not an error.
bool head_fused_form(const msr_handle* h) {
    static const bool sw_on = env_int("MSR_F16C_SW", 1) == 1;
    if (!h->fused_head || h->variant == MSR_PIX2PIX || !sw_on) return false;
    const ConvForm& cv = h->spade_forms[6][2].cv;
    const int r = h->S / 2;
    return cv.prec == PREC_F16C && cv.tile == TILE_256x128_PP && cv.ksplit == 1 && !cv.no_cross && kGenFilters[5] == 128 &&
           r >= 16 && (r & (r - 1)) == 0;
}

}  // namespace msr

// forms.hip — the form table: which kernel runs every conv layer of the generator and which weight image that kernel reads,
// fixed by the handle's batch, size and flags.  msr_load_weight and the planner both read it, so a layer's weights are always in
// the layout its launch expects.  The ONE unit that chooses a kernel (conv_kernel_for, conv_gbr_ranges) and reads the switches.
#include "host.h"

namespace msr {

const Switches& switches() {
    auto on = [](const char* name) { return env_int(name, 1) != 0; };
    static const int sw = env_int("MSR_F16C_SW", 1);     // fp6 is opt-in, and the A/B dispatches (0, 2) switch it off
    static const Switches s{on("MSR_PP_KSPLIT"), on("MSR_F16C_KSPLIT"), env_int("MSR_F16C_FP6", 0) == 1 && sw == 1, on("MSR_GBR"),
                            on("MSR_TILE_WALK"), on("MSR_FUSE_MOMENTS"), on("MSR_SMALLCIN_TILED"), sw};
    return s;
}

int conv_kernel_for(int prec, int tile, int ksplit, int wt_frag, int cin, int epi, int out_split) {
    const bool pp = tile == TILE_256x128_PP;
    const int sw = switches().f16c_sw;
    if (epi == EPI_RES_HEAD) return KERNEL_SW;                // the head epilogue exists in the stream kernel only
    if (prec == PREC_F32) return KERNEL_GENERIC;
    if (prec == PREC_BF16X3)                                  // by tile; else B fragments in VGPRs or the LDS-staged weight image
        return pp ? KERNEL_PP : tile == TILE_128x128_HALO ? KERNEL_HALO : tile == TILE_128x128_HALO16 ? KERNEL_HALO16
                  : wt_frag ? KERNEL_BVGPR : KERNEL_GENERIC;
    if (!pp || prec < PREC_F16X2 || prec > PREC_F16C6) return -1;   // the quantised forms exist on the 256 x 128 tile only
    if (prec == PREC_F16C6) return KERNEL_SW;
    if (prec != PREC_F16C || ksplit > 1) return KERNEL_PP;    // F16X2, FP8; f16c K ranges (+ split-K pass)
    // f16c whole tiles: conv_sw.hip takes the long-K main convs; the gamma|beta convs stay on the ping-pong kernel, where a second
    // wave on the SIMD hides their SPADE epilogue (and which alone writes the fp6 image).  MSR_F16C_SW = 0: all there, 2: all here.
    const bool stream = cin % 128 == 0 && !(epi == EPI_SPADE && out_split == OUT_F16C6) && (sw == 2 || (sw == 1 && epi != EPI_SPADE));
    return stream ? KERNEL_SW : KERNEL_PP;
}

// Work decomposition of conv_gb_resident: a work item = one 16 x 16 pixel tile x `nr` channel blocks; the N / 128 blocks of a pixel
// tile are cut into the fewest ranges (a power of two) that give every CU an item.  0 = the layer is not one for that kernel.
int conv_gbr_ranges(int B, int r, int N) {
    if (!switches().gbr || r < 16 || (r & (r - 1)) || N % 128) return 0;
    const int tiles_p = B * (r / 16) * (r / 16), tiles_n = N / 128;
    int ranges = 1;
    while (tiles_p * ranges < 256 && ranges * 2 <= tiles_n && tiles_n % (ranges * 2) == 0) ranges *= 2;
    if (tiles_p * ranges < 128) return 0;               // too few items even at one block per item
    // one block per item on half of the CUs: still ahead of the ping-pong K ranges + split-K epilogue + embedding launch at
    // r = 16 (26 against 38 us at B = 8), not at higher resolution where those launches fill the chip
    if (tiles_n / ranges < 2 && tiles_p * ranges < 256 && r > 16) return 0;
    return ranges;
}

// K split of the persistent ping-pong kernel for layers with fewer 16 x 16 x 128 tiles than CUs: whole chunk pairs
// per range, a power of two, as many ranges as it takes to give every CU a work item.  0 = the layer is not one for
// that kernel (it needs stride 1, r >= 16, Cin % 64 == 0, an input below the 2 GiB buffer-descriptor range and, split
// or not, at least `min_items` work items — below that the small-tile split-K kernels are faster).
static int pp_ksplit(int B, int rout, int N, int stride, int cin, long min_items = 128) {
    if (stride != 1 || rout < 16 || cin % 64 || N % 128) return 0;
    if ((size_t)B * (rout + 2) * (rout + 2) * cin * sizeof(float) >= ((size_t)1 << 31)) return 0;
    const long tiles = (long)B * (rout / 16) * (rout / 16) * (N / 128);
    if (tiles >= 256) return 1;
    if (!switches().pp_ksplit) return 0;
    const int pairs = cin / 64;
    int ks = 1;
    while (tiles * ks * 2 <= 256 && pairs % (ks * 2) == 0) ks *= 2;
    return tiles * ks >= min_items ? ks : 0;
}

// A conv form.  Its kernel follows from the rule above (cin: float slots per pixel of its input; out_split: the image an
// EPI_SPADE epilogue writes), its weight image from the precision (and, under bf16x3, from the fragment order).
ConvForm make_form(int prec, int tile, int ksplit, int cin, int epi, int out_split, int wt_frag, int no_cross) {
    ConvForm f;
    f.prec = prec; f.tile = tile; f.ksplit = ksplit; f.wt_frag = wt_frag; f.no_cross = no_cross;
    f.kernel = conv_kernel_for(prec, tile, ksplit, wt_frag, cin, epi, out_split);
    static const WeightImage kImage[] = {IMG_F32, IMG_BF16, IMG_F16, IMG_FP8, IMG_F16C, IMG_F16C6};   // by ConvPrecision
    f.img = prec == PREC_BF16X3 && wt_frag ? IMG_BF16_FRAG : kImage[prec];
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
    return make_form(prec, tile, ksplit > 0 ? ksplit : conv_pick_ksplit(M, N, ksteps, tile, prec), cin, epi, OUT_F32, wt_frag);
}

// out_split of a producer whose output feeds a conv in `prec`: the operand image that conv reads (kernels.h: the OutFormat of
// the same number)
static int split_for(int prec) { return prec; }
static_assert(OUT_BF16X3 == PREC_BF16X3 && OUT_F16X2 == PREC_F16X2 && OUT_BF8 == PREC_FP8 && OUT_F16C == PREC_F16C && OUT_F16C6 == PREC_F16C6, "");

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
    const Switches& sw = switches();
    const int B = h->B, PP = TILE_256x128_PP;
    auto fills = [&](int N) { return r >= 16 && N % 128 == 0 && (long)B * (r / 16) * (r / 16) * (N / 128) >= 256; };
    auto f16c_pp = [&](int N, int cin) { return sw.f16c_ksplit ? pp_ksplit(B, r, N, 1, cin) >= 1 : fills(N); };
    const bool gb8 = h->fp8 && fills(2 * C), cv8 = gb8 && fills(cout);
    const bool gbc = h->f16c && f16c_pp(2 * C, 128), cvc = gbc && C % 64 == 0 && f16c_pp(cout, C);
    SpadeForm s;
    s.hslots = gb8 ? fp8_pad(128) / 4 : 128;
    s.aslots = cv8 ? fp8_pad(C) / 4 : C;
    // The consumer first: its precision is the image the gamma|beta epilogue writes, and that conv's kernel depends on it.
    // The f16 mode asks for no cross terms on whole tiles, the stream kernel's form: a K-range launch runs the ping-pong
    // kernel, which has no such form and computes them (and so do whole tiles under MSR_F16C_SW=0: DESIGN.md, open follow-up).
    const int ks = pp_ksplit(B, r, cout, 1, C);
    const ConvForm cvf = make_form(PREC_F16C, PP, ks, C, epi, OUT_F32, 0, h->f16m && ks == 1);
    // the f16c6 consumer is the stream kernel, and only under the default dispatch (MSR_F16C_SW=1)
    const bool cv6 = cvc && (sw.f16c_fp6 || (h->cross6 && sw.f16c_sw == 1)) && cvf.kernel == KERNEL_SW && fills(cout) && fills(2 * C);
    if (cv8) s.cv = make_form(PREC_FP8, PP, 1, s.aslots, epi);
    else if (cv6) s.cv = make_form(PREC_F16C6, PP, 1, C, epi);
    else if (cvc) s.cv = cvf;
    else s.cv = conv_form(B, r, cout, 1, epi, h->prec, C);
    s.a_split = split_for(s.cv.prec);
    s.ranges = cvc && (!cv6 || h->cross6) ? conv_gbr_ranges(B, r, 2 * C) : 0;
    if (gb8) {
        s.gb = make_form(PREC_FP8, PP, 1, s.hslots, EPI_SPADE, s.a_split);
    } else if (s.ranges > 0) {
        s.gb = make_form(PREC_F16C6, PP, 1, 128, EPI_SPADE, s.a_split, 0, h->f16m);   // (its kernel is conv_gb_resident, not .kernel)
        s.gb.img = IMG_GBR;
    } else if (gbc) {
        s.gb = make_form(PREC_F16C, PP, pp_ksplit(B, r, 2 * C, 1, 128), 128, EPI_SPADE, s.a_split);   // > 1: K ranges
    } else {
        s.gb = conv_form(B, r, 2 * C, 1, EPI_SPADE, h->prec, 128);
        if (h->gb_f16x2 && s.gb.kernel == KERNEL_PP && s.gb.ksplit == 1) s.gb = make_form(PREC_F16X2, PP, 1, 128, EPI_SPADE, s.a_split);
    }
    s.h_split = split_for(s.gb.prec);
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
    if (!h->fused_head || h->variant == MSR_PIX2PIX || switches().f16c_sw != 1) return false;
    const ConvForm& cv = h->spade_forms[6][2].cv;
    const int r = h->S / 2;
    return cv.kernel == KERNEL_SW && cv.prec == PREC_F16C && cv.ksplit == 1 && !cv.no_cross && kGenFilters[5] == 128 &&
           r >= 16 && (r & (r - 1)) == 0;
}

}  // namespace msr

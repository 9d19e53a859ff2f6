// op_entries.hip — the kernel-level entries (msr_op_*): one kernel family each on caller-supplied device tensors, for the
// tests that check a kernel against its reference.
#include "host.h"

using namespace msr;

// What every conv entry binds after it has built its op: the output view (dense or zero-bordered, `oslots` float slots per
// pixel), the aux view (residual / the tensor SPADE normalises), the SPADE moments and, for a K split, the handle's split-K
// workspace.
static int bind_conv_entry(msr_handle* h, Op& op, float* out_dev, int out_padded, int oslots, const float* aux_dev,
                           int aux_shift, const float* mean_dev, const float* std_dev) {
    ConvParams& c = op.conv;
    const int rout = c.Hout, Cout = op.epi == EPI_SPADE ? c.N / 2 : c.N;
    if (out_padded) set_out_padded(c, out_dev, rout, rout, oslots);
    else set_out_dense(c, out_dev, rout, rout, oslots);
    if (op.epi != EPI_BIAS) set_aux_dense(c, aux_dev, rout >> aux_shift, Cout, aux_shift);
    c.mean = mean_dev; c.stdv = std_dev;
    if (c.ksplit > 1) {
        int rc = ensure_conv_partial(h, (size_t)c.ksplit * c.B * rout * rout * c.N);
        if (rc) return rc;
        c.partial = h->conv_partial;
    }
    return MSR_OK;
}

extern "C" {

static int op_conv_impl(msr_handle* h, const float* in_dev, const float* wt_dev, const float* bias_dev, float* out_dev,
                        int32_t B, int32_t rout, int32_t Cin, int32_t N, int32_t stride, int32_t epilogue,
                        const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev,
                        int32_t out_padded, int32_t tile, int prec, int out_split, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!in_dev || !wt_dev || !bias_dev || !out_dev || B < 1 || rout < 1 || (stride != 1 && stride != 2))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3: bad argument");
    if (epilogue < EPI_BIAS || epilogue > EPI_SPADE || (epilogue != EPI_BIAS && !aux_dev) ||
        (epilogue == EPI_SPADE && (!mean_dev || !std_dev)))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3: epilogue %d needs aux / mean / std", epilogue);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    Padded in; in.base = const_cast<float*>(in_dev); in.r = rout * stride; in.C = Cin;
    Op op = conv_op(in, Cin, wt_dev, bias_dev, B, rout, N, stride, epilogue, conv_form(B, rout, N, stride, epilogue, prec, Cin));
    op.conv.out_split = (epilogue == EPI_SPADE && out_split) ? OUT_BF16X3 : OUT_F32;
    if (tile >= 0) {
        op.tile = tile & 0x3F;
        if (tile & 0x80) op.conv.prec = PREC_F16X2;            // operands are split-fp16 words (ping-pong tile only)
        op.conv.wt_frag = (tile & 0x40) ? 1 : 0;
        op.conv.ksplit = (tile >> 8) > 0 ? (tile >> 8) : 1;    // explicit tile: explicit split (default none)
        op.kernel = conv_kernel_for(op.conv.prec, op.tile, op.conv.ksplit, op.conv.wt_frag, Cin, epilogue, op.conv.out_split);
    }
    int rc = bind_conv_entry(h, op, out_dev, out_padded, epilogue == EPI_SPADE ? N / 2 : N, aux_dev, aux_shift, mean_dev, std_dev);
    if (rc) return rc;
    hipError_t e = launch_conv(op.conv, epilogue, op.kernel, op.tile, (hipStream_t)stream);
    if (e != hipSuccess) return fail(h, MSR_ERR_INVALID, "conv launch rejected (shape not tileable?): %s", hipGetErrorString(e));
    return MSR_OK;
}

int msr_op_conv3x3(msr_handle* h, const float* in_dev, const float* wt_dev, const float* bias_dev, float* out_dev,
                   int32_t B, int32_t rout, int32_t Cin, int32_t N, int32_t stride, int32_t epilogue,
                   const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev,
                   int32_t out_padded, int32_t tile, void* stream) {
    return op_conv_impl(h, in_dev, wt_dev, bias_dev, out_dev, B, rout, Cin, N, stride, epilogue, aux_dev, aux_shift,
                        mean_dev, std_dev, out_padded, tile, PREC_F32, 0, stream);
}

int msr_op_conv3x3_bf16x3(msr_handle* h, const float* in_dev, const float* wt_dev, const float* bias_dev,
                          float* out_dev, int32_t B, int32_t rout, int32_t Cin, int32_t N, int32_t stride,
                          int32_t epilogue, const float* aux_dev, int32_t aux_shift, const float* mean_dev,
                          const float* std_dev, int32_t out_padded, int32_t out_split, int32_t tile, void* stream) {
    if (tile < 0) return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_bf16x3 needs an explicit tile (the weight layout depends on it)");
    if ((tile & 0x3F) == TILE_128x128_K16) return fail(h, MSR_ERR_INVALID, "the bf16x3 path has no 16-channel K-step tile");
    return op_conv_impl(h, in_dev, wt_dev, bias_dev, out_dev, B, rout, Cin, N, stride, epilogue, aux_dev, aux_shift,
                        mean_dev, std_dev, out_padded, tile, PREC_BF16X3, out_split, stream);
}

int msr_op_conv_affine(msr_handle* h, const float* in_dev, int32_t in_px, int32_t in_py, int32_t in_pb, const float* wt_dev,
                       const float* scale_dev, const float* shift_dev, float* out_dev, int32_t out_off, int32_t out_px,
                       int32_t out_py, int32_t out_pb, int32_t B, int32_t rout, int32_t Cin, int32_t N, int32_t KH, int32_t KW,
                       int32_t stride, int32_t act, float slope, int32_t tile, void* stream) {
    // Everything is checked before the handle or the device is touched (h == nullptr: the message goes to msr_last_error(NULL)),
    // so that what the kernel has no instantiation for is refused on a machine without a device too.
    if (!in_dev || !wt_dev || !shift_dev || !out_dev)
        return fail(h, MSR_ERR_INVALID, "msr_op_conv_affine: null argument (only scale_dev may be NULL)");
    if (B < 1 || rout < 1 || (rout & (rout - 1)) || KH < 1 || KW < 1 || KH > 8 || KW > 8 || (stride != 1 && stride != 2) || act < 0 ||
        act > 2)
        return fail(h, MSR_ERR_INVALID, "msr_op_conv_affine: bad argument (B >= 1, rout a power of two, 1 <= KH, KW <= 8, stride "
                    "1 | 2, act 0..2): B=%d rout=%d KH=%d KW=%d stride=%d act=%d", B, rout, KH, KW, stride, act);
    if (tile < -1 || (tile >= 0 && ((tile & 0xFF) > TILE_64x64 || (tile >> 8) > 256)))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv_affine: tile 0x%x is not -1 or (0 | 1) + 256 * ksplit", tile);
    if (Cin < 32 || Cin % 32 || N < 64 || N % 64)
        return fail(h, MSR_ERR_INVALID, "msr_op_conv_affine: Cin = %d must be a multiple of 32 (the K-step) and N = %d of 64", Cin, N);
    ConvForm f = conv_form(B, rout, N, stride, EPI_AFFINE, PREC_F32, Cin, KH * KW);
    if (tile >= 0) f = make_form(PREC_F32, tile & 0xFF, (tile >> 8) > 0 ? (tile >> 8) : 1, Cin, EPI_AFFINE);
    const int steps = KH * KW * (Cin / 32);
    if (f.tile == TILE_128x128 && N % 128)
        return fail(h, MSR_ERR_INVALID, "msr_op_conv_affine: the 128 x 128 tile needs N %% 128 == 0 (N = %d)", N);
    if (f.ksplit < 1 || f.ksplit > steps)      // a K range without a step would still run the kernel's last step
        return fail(h, MSR_ERR_INVALID, "msr_op_conv_affine: ksplit %d exceeds the %d K-steps of the shape", f.ksplit, steps);
    // 16-byte loads of the input, float4 stores of the split-K pass; the kernels index with 32-bit offsets
    if (in_px < Cin || in_px % 4 || in_py % 4 || in_pb % 4 || in_py < 0 || in_pb < 0 || ((uintptr_t)in_dev & 15) || ((uintptr_t)wt_dev & 15))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv_affine: input pitches (%d, %d, %d) must be multiples of 4 floats with in_px >= Cin, "
                    "in_dev and wt_dev 16-byte aligned", in_px, in_py, in_pb);
    if (out_off < 0 || out_px < N || out_px % 4 || out_py % 4 || out_pb % 4 || out_off % 4 || out_py < 0 || out_pb < 0 ||
        ((uintptr_t)out_dev & 15) || ((uintptr_t)shift_dev & 15) || ((uintptr_t)scale_dev & 15))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv_affine: output offset and pitches (%d; %d, %d, %d) must be multiples of 4 floats with "
                    "out_px >= N, out_dev, scale_dev and shift_dev 16-byte aligned", out_off, out_px, out_py, out_pb);
    const int64_t rin = (int64_t)(rout - 1) * stride + KH, cin_last = (int64_t)(rout - 1) * stride + KW;
    const int64_t in_span = (int64_t)(B - 1) * in_pb + (rin - 1) * in_py + (cin_last - 1) * in_px + Cin;
    const int64_t out_span = out_off + (int64_t)(B - 1) * out_pb + (int64_t)(rout - 1) * (out_py + out_px) + N;
    if (in_span >= ((int64_t)1 << 31) || out_span >= ((int64_t)1 << 31) || (int64_t)KH * KW * N * Cin >= ((int64_t)1 << 31))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv_affine: the tensors exceed the kernel's 32-bit element offsets");
    if (!h) return fail(nullptr, MSR_ERR_INVALID, "msr_op_conv_affine: null handle");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    Op op; op.type = OP_CONV; op.epi = EPI_AFFINE;        // filled as plan_pix2pix's igemm lambda fills it
    ConvParams& c = op.conv;
    c.in = in_dev; c.wt = wt_dev; c.bias = shift_dev; c.scale = scale_dev; c.act = act; c.slope = slope;
    c.B = B; c.Hout = rout; c.Wout = rout; c.Cin = Cin; c.N = N; c.KH = KH; c.KW = KW; c.stride = stride;
    c.in_px = in_px; c.in_py = in_py; c.in_pb = in_pb;
    c.prec = f.prec; c.ksplit = f.ksplit;
    op.tile = f.tile; op.kernel = f.kernel;
    c.out = out_dev; c.out_off = out_off; c.out_px = out_px; c.out_py = out_py; c.out_pb = out_pb;
    if (c.ksplit > 1) {
        int rc = ensure_conv_partial(h, (size_t)c.ksplit * B * rout * rout * N);
        if (rc) return rc;
        c.partial = h->conv_partial;
    }
    hipError_t e = launch_conv(c, EPI_AFFINE, op.kernel, op.tile, (hipStream_t)stream);
    if (e != hipSuccess) return fail(h, MSR_ERR_INVALID, "msr_op_conv_affine: launch rejected: %s", hipGetErrorString(e));
    return MSR_OK;
}

int msr_op_conv3x3_f16c(msr_handle* h, const float* in_dev, const float* wt_dev, const int32_t* wexp_dev,
                        const float* bias_dev, float* out_dev, int32_t B, int32_t rout, int32_t Cin, int32_t N,
                        int32_t epilogue, const float* aux_dev, int32_t aux_shift, const float* mean_dev,
                        const float* std_dev, int32_t out_padded, int32_t out_mode_bits, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    // out_mode_bits = out_mode | 256 * ksplit | 0x10000 (no cross terms)
    const int out_mode = out_mode_bits & 0xFF, ksplit = (out_mode_bits >> 8) & 0xFF, no_cross = (out_mode_bits >> 16) & 1;
    if (out_mode_bits < 0 || (out_mode_bits >> 17))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_f16c: unknown bits in out_mode 0x%x", out_mode_bits);
    if (!in_dev || !wt_dev || !bias_dev || !out_dev || B < 1 || rout < 16 || Cin % 64 || N % 128)
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_f16c: bad argument (Cin %% 64, N %% 128, rout >= 16)");
    // wexp_dev == nullptr: the operands are f16c6 images (fp6 pieces, scales inside; stream kernel, bias / residual epilogues)
    if (!wexp_dev && (epilogue == EPI_SPADE || Cin % 128 || ksplit > 1 || no_cross))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_f16c: the f16c6 form takes whole-tile bias / residual launches and Cin %% 128 == 0");
    if (epilogue < EPI_BIAS || epilogue > EPI_SPADE || (epilogue != EPI_BIAS && !aux_dev) ||
        (epilogue == EPI_SPADE && (!mean_dev || !std_dev)) || (out_mode != OUT_F32 && out_mode != OUT_BF16X3 && out_mode != OUT_F16C && out_mode != OUT_F16C6) ||
        (out_mode != OUT_F32 && epilogue != EPI_SPADE))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_f16c: bad epilogue / output mode");
    // K ranges: whole chunk pairs per range (launch_pp); the split-K epilogue writes fp32, split-bf16 or the f16c image
    if (ksplit > 1 && ((ksplit & (ksplit - 1)) || (Cin / 64) % ksplit || out_mode == OUT_F16C6))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_f16c: ksplit %d must be a power of two dividing Cin / 64 = %d (out_mode 0, 1, 4)",
                    ksplit, Cin / 64);
    // no cross terms: the stream kernel's form only (whole tiles, bias / residual, Cin % 128 == 0, power-of-two rout)
    if (no_cross && (ksplit > 1 || epilogue == EPI_SPADE || Cin % 128 || (rout & (rout - 1))))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_f16c: no-cross takes whole-tile bias / residual launches with Cin %% 128 == 0");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    Padded in; in.base = const_cast<float*>(in_dev); in.r = rout; in.C = Cin;
    const int out_split = epilogue == EPI_SPADE ? out_mode : OUT_F32;
    Op op = conv_op(in, Cin, wt_dev, bias_dev, B, rout, N, 1, epilogue,
                    make_form(wexp_dev ? PREC_F16C : PREC_F16C6, TILE_256x128_PP, ksplit > 1 ? ksplit : 1, Cin, epilogue, out_split, 0, no_cross));
    // no-cross is the stream kernel's form alone, whatever the rule says: under MSR_F16C_SW = 0 it names the ping-pong kernel,
    // which has no such form and would silently compute the cross terms
    if (no_cross) op.kernel = KERNEL_SW;
    op.conv.wexp = wexp_dev;
    op.conv.out_split = out_split;
    int rc = bind_conv_entry(h, op, out_dev, out_padded, epilogue == EPI_SPADE ? N / 2 : N, aux_dev, aux_shift, mean_dev, std_dev);
    if (rc) return rc;
    hipError_t e = launch_conv(op.conv, epilogue, op.kernel, op.tile, (hipStream_t)stream);
    if (e != hipSuccess) return fail(h, MSR_ERR_INVALID, "f16c conv launch rejected: %s", hipGetErrorString(e));
    return MSR_OK;
}

int msr_op_conv3x3_f16c_head(msr_handle* h, const float* in_dev, const float* wt_dev, const int32_t* wexp_dev,
                             const float* bias_dev, int32_t B, int32_t rout, int32_t Cin, int32_t N, const float* aux_dev,
                             int32_t aux_shift, const float* head_kernel_host, float head_bias, float* out_dev,
                             float* partial_dev, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!in_dev || !wt_dev || !wexp_dev || !bias_dev || !aux_dev || !head_kernel_host || !out_dev || B < 1)
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_f16c_head: null argument");
    if (N != 128 || Cin < 128 || Cin % 128 || rout < 16 || (rout & (rout - 1)) || aux_shift < 0 || aux_shift > 1)
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_f16c_head: N must be 128, Cin a multiple of 128, rout >= 16 a power of two "
                    "(the stream kernel's whole-tile form), aux_shift 0 | 1");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    Padded in; in.base = const_cast<float*>(in_dev); in.r = rout; in.C = Cin;
    Op op = conv_op(in, Cin, wt_dev, bias_dev, B, rout, N, 1, EPI_RES_HEAD, make_form(PREC_F16C, TILE_256x128_PP, 1, Cin, EPI_RES_HEAD));
    op.conv.wexp = wexp_dev;
    const std::vector<float> wfrag = build_head_wfrag(head_kernel_host);
    float *wd = nullptr, *pd = partial_dev;
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipMalloc(&wd, wfrag.size() * sizeof(float)));
    hipError_t e = hipMemcpy(wd, wfrag.data(), wfrag.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && !pd) e = hipMalloc(&pd, (size_t)B * rout * rout * 32 * sizeof(float));
    bool rejected = false;
    if (e == hipSuccess) {
        set_out_dense(op.conv, pd, rout, rout, 32);
        set_aux_dense(op.conv, aux_dev, rout >> aux_shift, N, aux_shift);
        op.conv.mean = wd;
        e = launch_conv(op.conv, EPI_RES_HEAD, op.kernel, op.tile, s);
        rejected = e != hipSuccess;
    }
    if (e == hipSuccess) e = launch_head_gather(pd, head_bias, out_dev, B, rout, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    hipFree(wd);
    if (pd != partial_dev) hipFree(pd);
    if (rejected) return fail(h, MSR_ERR_INVALID, "f16c head conv launch rejected: %s", hipGetErrorString(e));
    if (e != hipSuccess) return fail(h, MSR_ERR_DEVICE, "msr_op_conv3x3_f16c_head failed: %s", hipGetErrorString(e));
    return MSR_OK;
}

static int op_spade_gbr_impl(msr_handle* h, const float* src_dev, int32_t S, const float* we_dev, const float* be_dev,
                             const float* wt_dev, const float* bias_dev, float* out_dev, int32_t B, int32_t r, int32_t N,
                             const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev, int no_cross,
                             int out_split, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!src_dev || !we_dev || !be_dev || !wt_dev || !bias_dev || !out_dev || !aux_dev || !mean_dev || !std_dev || B < 1 ||
        r < 16 || (r & (r - 1)) || S < r || S % r || N % 128 || aux_shift < 0 || aux_shift > 1)
        return fail(h, MSR_ERR_INVALID, "msr_op_spade_gbr: bad argument (r >= 16 a power of two, S a multiple of r, N %% 128 == 0)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int C = N / 2, rx = r >> aux_shift;
    GbrParams q{};
    q.src = src_dev; q.we = we_dev; q.be = be_dev; q.S = S; q.f = S / r; q.o = (S / r) / 2;
    q.wt = wt_dev; q.bias = bias_dev;
    set_aux_dense(q, aux_dev, rx, C, aux_shift);
    q.mean = mean_dev; q.stdv = std_dev;
    set_out_padded(q, out_dev, r, r, C);
    q.out_split = out_split; q.slope = 0.2f; q.B = B; q.r = r; q.N = N; q.no_cross = no_cross;
    int ranges = conv_gbr_ranges(B, r, N);       // the planner's split; a layer it would not take runs one item per pixel tile
    if (ranges < 1) ranges = 1;
    // the embedding kernel as fp16 MFMA operands (msr_load_weight builds this image once per layer; this test entry per call)
    std::vector<float> we_host(9 * 2 * 128), e16(4096);
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(h, hipMemcpy(we_host.data(), we_dev, we_host.size() * sizeof(float), hipMemcpyDeviceToHost));
    conv_gbr_embed_image(we_host.data(), e16.data());
    float* e16_dev = nullptr;
    HIPCHK(h, hipMalloc(&e16_dev, e16.size() * sizeof(float)));
    hipError_t e = hipMemcpy(e16_dev, e16.data(), e16.size() * sizeof(float), hipMemcpyHostToDevice);
    q.we16 = e16_dev;
    if (e == hipSuccess) e = launch_conv_gbr(q, ranges, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    hipFree(e16_dev);
    if (e != hipSuccess) return fail(h, MSR_ERR_INVALID, "conv_gb_resident launch rejected: %s", hipGetErrorString(e));
    return MSR_OK;
}

int msr_op_spade_gbr(msr_handle* h, const float* src_dev, int32_t S, const float* we_dev, const float* be_dev,
                     const float* wt_dev, const float* bias_dev, float* out_dev, int32_t B, int32_t r, int32_t N,
                     const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev, void* stream) {
    return op_spade_gbr_impl(h, src_dev, S, we_dev, be_dev, wt_dev, bias_dev, out_dev, B, r, N, aux_dev, aux_shift, mean_dev,
                             std_dev, 0, 4, stream);
}

int msr_op_spade_gbr_f16(msr_handle* h, const float* src_dev, int32_t S, const float* we_dev, const float* be_dev,
                         const float* wt_dev, const float* bias_dev, float* out_dev, int32_t B, int32_t r, int32_t N,
                         const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev, void* stream) {
    return op_spade_gbr_impl(h, src_dev, S, we_dev, be_dev, wt_dev, bias_dev, out_dev, B, r, N, aux_dev, aux_shift, mean_dev,
                             std_dev, 1, 4, stream);
}

int msr_op_spade_gbr_f16c6(msr_handle* h, const float* src_dev, int32_t S, const float* we_dev, const float* be_dev,
                           const float* wt_dev, const float* bias_dev, float* out_dev, int32_t B, int32_t r, int32_t N,
                           const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev, void* stream) {
    return op_spade_gbr_impl(h, src_dev, S, we_dev, be_dev, wt_dev, bias_dev, out_dev, B, r, N, aux_dev, aux_shift, mean_dev,
                             std_dev, 0, 5, stream);
}

int msr_op_conv_smallcin(msr_handle* h, const float* src_dev, int32_t S, const float* w_dev, const float* bias_dev,
                         float* out_dev, int32_t B, int32_t Hout, int32_t Cout, int32_t map, int32_t act, float slope,
                         int32_t out_split, int32_t out_padded, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    // the kernel reads any out_split outside 2, 3, 4 as split-bf16: only the five formats the planner writes are accepted
    if (!src_dev || !w_dev || !out_dev || B < 1 || Hout < 1 || (Cout != 64 && Cout != 128) || map < 0 || map > 1 || act < 0 ||
        act > 2 || out_split < OUT_F32 || out_split > OUT_F16C || out_padded < 0 || out_padded > 1 ||
        (map == 0 && S != 2 * Hout) || (map == 1 && (S < Hout || S % Hout)))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv_smallcin: bad argument (Cout 64 | 128, map 0: S = 2 Hout, map 1: S a "
                    "multiple of Hout, act 0..2, out_split 0..4)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    SmallCinParams p{};
    p.src = src_dev; p.w = w_dev; p.bias = bias_dev;
    p.B = B; p.S = S; p.Hout = Hout; p.Cout = Cout;
    if (map == 0) { p.ay = 2; p.cy = 0; p.lim = S; p.f = 1; p.o = 0; }                       // encoder ds1: stride-2 SAME
    else { p.ay = 1; p.cy = -1; p.lim = Hout; p.f = S / Hout; p.o = (S / Hout) / 2; }       // SPADE mask embedding
    const int slots = out_split == OUT_BF8 ? fp8_pad(Cout) / 4 : Cout;       // bf8: one byte per channel, padded to 128
    if (out_padded) set_out_padded(p, out_dev, Hout, Hout, slots);
    else set_out_dense(p, out_dev, Hout, Hout, slots);
    p.act = act; p.slope = slope; p.out_split = out_split;
    hipError_t e = launch_conv_smallcin(p, (hipStream_t)stream);
    if (e != hipSuccess) return fail(h, MSR_ERR_INVALID, "conv_smallcin launch rejected: %s", hipGetErrorString(e));
    return MSR_OK;
}

int msr_op_norm_act(msr_handle* h, const float* x_dev, const float* mean_dev, const float* std_dev, const float* gamma_dev,
                    const float* beta_dev, float* out_dev, int32_t B, int32_t H, int32_t W, int32_t C, float slope,
                    int32_t out_padded, int32_t out_split, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!x_dev || !mean_dev || !std_dev || !gamma_dev || !beta_dev || !out_dev || B < 1 || H < 1 || W < 1 || C < 4 || C % 4 ||
        out_padded < 0 || out_padded > 1 || out_split < OUT_F32 || out_split > OUT_BF16X3 || (out_split && C % 32))
        return fail(h, MSR_ERR_INVALID, "msr_op_norm_act: bad argument (C a multiple of 4, of 32 for split output; "
                    "out_padded, out_split 0 | 1)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    NormActParams p{};
    p.x = x_dev; p.mean = mean_dev; p.stdv = std_dev; p.gamma = gamma_dev; p.beta = beta_dev;
    p.B = B; p.H = H; p.W = W; p.C = C; p.slope = slope; p.out_split = out_split;
    if (out_padded) set_out_padded(p, out_dev, H, W, C);
    else set_out_dense(p, out_dev, H, W, C);
    hipError_t e = launch_norm_act(p, (hipStream_t)stream);
    if (e != hipSuccess) return fail(h, MSR_ERR_INVALID, "norm_act launch rejected: %s", hipGetErrorString(e));
    return MSR_OK;
}

int msr_op_dense(msr_handle* h, const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int32_t B,
                 int32_t K, int32_t N, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!x_dev || !w_dev || !y_dev || B < 1 || B > 16 || K < 1 || N < 4 || N % 4 || (long)B * N >= (1L << 31))
        return fail(h, MSR_ERR_INVALID, "msr_op_dense: bad argument (1 <= B <= 16, K >= 1, N a multiple of 4)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    float* partial = nullptr;
    HIPCHK(h, hipMalloc(&partial, dense_partial_floats(B, K, N) * sizeof(float)));
    hipError_t e = launch_dense(x_dev, w_dev, bias_dev, partial, y_dev, B, K, N, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    hipFree(partial);
    if (e != hipSuccess) return fail(h, MSR_ERR_DEVICE, "msr_op_dense failed: %s", hipGetErrorString(e));
    return MSR_OK;
}

int msr_op_latent(msr_handle* h, const float* mv_dev, const float* eps_dev, float* z_dev, int32_t B, int32_t L,
                  int32_t sampler, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!mv_dev || !z_dev || B < 1 || L < 1 || sampler < 0 || sampler > 1 || (sampler && !eps_dev) || (long)B * L >= (1L << 31))
        return fail(h, MSR_ERR_INVALID, "msr_op_latent: bad argument (sampler 0 | 1, eps needed by sampler 1)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipError_t e = launch_latent(mv_dev, eps_dev, z_dev, B, L, sampler, (hipStream_t)stream);
    if (e != hipSuccess) return fail(h, MSR_ERR_INVALID, "latent launch rejected: %s", hipGetErrorString(e));
    return MSR_OK;
}

int msr_op_head(msr_handle* h, const float* x_dev, const float* kernel_host, float bias, float* out_dev, int32_t B,
                int32_t r, int32_t C, float slope, int32_t variant, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!x_dev || !kernel_host || !out_dev || B < 1 || r < 16 || r % 16 || C < 16 || C % 16 || variant < 0 || variant > 1)
        return fail(h, MSR_ERR_INVALID, "msr_op_head: bad argument (r and C multiples of 16, variant 0 | 1)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const std::vector<float> weff = variant ? head_weff_transpose(kernel_host, C) : head_weff_upconv(kernel_host, C);
    float* wd = nullptr;
    HIPCHK(h, hipMalloc(&wd, weff.size() * sizeof(float)));
    hipError_t e = hipMemcpy(wd, weff.data(), weff.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_head(x_dev, wd, bias, out_dev, B, r, C, slope, variant, 0, 0, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    hipFree(wd);
    if (e != hipSuccess) return fail(h, MSR_ERR_DEVICE, "msr_op_head failed: %s", hipGetErrorString(e));
    return MSR_OK;
}

int msr_op_moments(msr_handle* h, const float* x_dev, int32_t G, int32_t P, int32_t C, float eps, float* mean_dev,
                   float* std_dev, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!x_dev || !mean_dev || !std_dev || G < 1 || G > 65535 || P < 1 || C < 32 || C % 32 || !(eps >= 0.f))
        return fail(h, MSR_ERR_INVALID, "msr_op_moments: bad argument (G in [1, 65535], P >= 1, C a multiple of 32, eps >= 0)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    double* partial = nullptr;
    HIPCHK(h, hipMalloc(&partial, (size_t)G * moments_chunks(G, P) * C * 2 * sizeof(double)));
    hipError_t e = launch_moments(x_dev, G, P, C, eps, partial, mean_dev, std_dev, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    hipFree(partial);
    if (e != hipSuccess) return fail(h, MSR_ERR_DEVICE, "msr_op_moments failed: %s", hipGetErrorString(e));
    return MSR_OK;
}

int64_t msr_quantize_e4m3(const float* host, int64_t n, uint8_t* out) {
    if (!host || !out || n < 0) return -1;
    for (int64_t i = 0; i < n; ++i) out[i] = msr_f32_to_e4m3(host[i]);
    return n;
}

int msr_op_conv3x3_fp8(msr_handle* h, const void* in_dev, const void* wt_dev, const int32_t* wexp_dev, const float* bias_dev,
                       float* out_dev, int32_t B, int32_t rout, int32_t Cpad, int32_t N, int32_t epilogue,
                       const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev,
                       int32_t out_padded, int32_t out_mode, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!in_dev || !wt_dev || !wexp_dev || !bias_dev || !out_dev || B < 1 || rout < 16 || (Cpad != 128 && Cpad % 256) ||
        N % 128)
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_fp8: bad argument (Cpad 128 or a multiple of 256, N %% 128, rout >= 16)");
    if (epilogue < EPI_BIAS || epilogue > EPI_SPADE || (epilogue != EPI_BIAS && !aux_dev) ||
        (epilogue == EPI_SPADE && (!mean_dev || !std_dev)) || (out_mode != OUT_F32 && out_mode != OUT_BF16X3 && out_mode != OUT_BF8) ||
        (out_mode != OUT_F32 && epilogue != EPI_SPADE))
        return fail(h, MSR_ERR_INVALID, "msr_op_conv3x3_fp8: bad epilogue / output mode");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    Padded in; in.base = const_cast<float*>(static_cast<const float*>(in_dev)); in.r = rout; in.C = Cpad / 4;
    Op op = conv_op(in, Cpad, static_cast<const float*>(wt_dev), bias_dev, B, rout, N, 1, epilogue,
                    make_form(PREC_FP8, TILE_256x128_PP, 1, Cpad / 4, epilogue, epilogue == EPI_SPADE ? out_mode : OUT_F32));
    op.conv.wexp = wexp_dev;
    op.conv.out_split = epilogue == EPI_SPADE ? out_mode : OUT_F32;
    const int Cout = epilogue == EPI_SPADE ? N / 2 : N;
    int rc = bind_conv_entry(h, op, out_dev, out_padded, out_mode == OUT_BF8 ? fp8_pad(Cout) / 4 : Cout, aux_dev, aux_shift, mean_dev,
                             std_dev);
    if (rc) return rc;
    hipError_t e = launch_conv(op.conv, epilogue, op.kernel, op.tile, (hipStream_t)stream);
    if (e != hipSuccess) return fail(h, MSR_ERR_INVALID, "fp8 conv launch rejected: %s", hipGetErrorString(e));
    return MSR_OK;
}

int msr_op_split_bf16(msr_handle* h, const float* in_dev, float* out_dev, int64_t count, void* stream) {
    if (!h || !in_dev || !out_dev || count < 0) return MSR_ERR_INVALID;
    if (count % 32) return fail(h, MSR_ERR_INVALID, "msr_op_split_bf16: count must be a multiple of 32 (channel chunks)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, launch_split_bf16(in_dev, out_dev, (long)count, (hipStream_t)stream));
    return MSR_OK;
}

int msr_op_range_scan(msr_handle* h, const void* img_dev, int32_t format, int32_t B, int32_t r, int32_t C, int32_t padded,
                      msr_range_stat* out_stat, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!img_dev || !out_stat) return fail(h, MSR_ERR_INVALID, "msr_op_range_scan: null argument");
    if (format < OUT_F16X2 || format > OUT_F16C6) return fail(h, MSR_ERR_INVALID, "msr_op_range_scan: format %d is not 2, 3, 4 or 5", format);
    if (B < 1 || r < 1 || C < 32 || C % 32 || (int64_t)B * r > (1 << 24) || (int64_t)r * C > (1 << 24))
        return fail(h, MSR_ERR_INVALID, "msr_op_range_scan: bad shape B=%d r=%d C=%d (C a multiple of 32)", B, r, C);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const RangeScanItem item{img_dev, format, B, r, C, format == OUT_BF8 ? fp8_pad(C) : 4 * C, padded != 0, 0};
    char* buf = nullptr;     // [record | item]
    HIPCHK(h, hipMalloc(&buf, sizeof(RangeScanRecord) + sizeof(RangeScanItem)));
    RangeScanRecord rec{};
    hipError_t e = hipMemsetAsync(buf, 0, sizeof(RangeScanRecord), s);
    if (e == hipSuccess) e = hipMemcpyAsync(buf + sizeof(RangeScanRecord), &item, sizeof item, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = launch_range_scan(reinterpret_cast<const RangeScanItem*>(buf + sizeof(RangeScanRecord)), 1,
                              reinterpret_cast<RangeScanRecord*>(buf), B * r, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(&rec, buf, sizeof rec, hipMemcpyDeviceToHost);
    hipFree(buf);
    if (e != hipSuccess) return fail(h, MSR_ERR_DEVICE, "msr_op_range_scan failed: %s", hipGetErrorString(e));
    range_fill(out_stat, "", format, -1, rec);
    return MSR_OK;
}

}  // extern "C"

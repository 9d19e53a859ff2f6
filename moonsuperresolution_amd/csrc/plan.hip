// plan.hip — the launch plan: the ops of one generator(call) with their workspace (plan_spade, plan_pix2pix), the split-K
// and moments workspaces (ensure_plan, ensure_conv_partial) and the tensors the activation-range scan reads
// (build_range_plan).
#include "host.h"

namespace msr {

// `written`: the float slots per pixel the buffer's producer writes (-1: all C).  The rest stays zero from here on, and the
// consumer may read it (msr_debug_fill_workspace keeps out of it).
static int alloc_padded(msr_handle* h, const std::string& key, int r, int C, Padded* out, int written = -1) {
    out->r = r; out->C = C;
    h->dev_padded[key] = {r, C, written < 0 ? C : written};
    return dev_alloc(h, key, (size_t)h->B * (r + 2) * (r + 2) * C, true, &out->base);
}

// A 3x3 conv of `cin` channels (in.C float slots per pixel: fewer for the byte-per-channel fp8 input) in form f.  The
// output format (out_split) is the caller's: a SPADE output feeds a conv whose form decides it.
Op conv_op(const Padded& in, int cin, const float* wt, const float* bias, int B, int rout, int N, int stride, int epi,
           const ConvForm& f) {
    Op op; op.type = OP_CONV; op.epi = epi; op.tile = f.tile; op.kernel = f.kernel;
    ConvParams& c = op.conv;
    c.in = stride == 1 ? in.base : in.base + in.interior();
    c.wt = wt; c.bias = bias;
    c.B = B; c.Hout = rout; c.Wout = rout; c.Cin = in.C; c.N = N;
    c.KH = 3; c.KW = 3; c.stride = stride;
    c.in_px = in.C; c.in_py = in.py(); c.in_pb = in.pb();
    c.slope = 0.2f;
    c.prec = f.prec; c.ksplit = f.ksplit; c.wt_frag = f.wt_frag; c.no_cross = f.no_cross;
    c.partial = nullptr;   // bound to the handle's workspace at launch
    op.flops = 2.0 * B * rout * rout * (double)cin * N * 9;
    return op;
}

static Op moments_op(const float* x, int G, int P, int C, float eps, float* mean, float* stdv) {
    Op op; op.type = OP_MOMENTS;
    op.mom = {x, G, P, C, eps, mean, stdv};
    op.bytes = (double)G * P * C * 4;
    return op;
}

// A split-K conv whose output feeds a normalisation takes the moments in its own epilogue (splitk_epilogue_mom_kernel).
static bool fuse_moments_into_splitk(Op& cv, int G, float eps, float* mean, float* stdv) {
    if (cv.type != OP_CONV || cv.conv.ksplit <= 1 || (cv.epi != EPI_BIAS && cv.epi != EPI_RES) || cv.conv.N % 32 ||
        !switches().fuse_moments)
        return false;
    cv.conv.mom_mean = mean; cv.conv.mom_std = stdv; cv.conv.mom_eps = eps; cv.conv.mom_G = G;
    return true;
}

static int plan_spade(msr_handle* h) {
    const int S = h->S, B = h->B, L = h->L;
    char n[160];
    int rc;
    auto need = [&](const std::string& k) -> float* { return D(h, k); };
    size_t mom_doubles = 0;
    auto mom_need = [&](int G, int P, int C) { mom_doubles = std::max(mom_doubles, (size_t)G * moments_chunks(G, P) * C * 2); };

    // ---------------- encoder (networks.py:8-34) ----------------
    Padded e_in;   // input of the next strided conv
    rc = alloc_padded(h, "ws.enc.p1", S / 2, 64, &e_in); if (rc) return rc;
    {
        Op op; op.type = OP_SMALLCIN; op.src_is_input = true;
        SmallCinParams& p = op.sc;
        p.w = need("enc.ds1.kernel"); p.bias = nullptr;
        p.B = B; p.S = S; p.Hout = S / 2; p.Cout = 64;
        p.ay = 2; p.cy = 0; p.lim = S; p.f = 1; p.o = 0;
        set_out_padded(p, e_in);
        p.act = 2; p.slope = 0.2f;
        p.out_split = h->prec == PREC_BF16X3 ? OUT_BF16X3 : OUT_F32;
        op.flops = 2.0 * B * (S / 2) * (S / 2) * 18.0 * 64;
        h->ops.push_back(op);
    }
    float* flat = nullptr;
    const int rlast = S / 32;
    for (int i = 2; i <= 5; ++i) {
        const int c = kEncChannels[i - 1], r = S >> i;
        float* raw; float *mean, *stdv;
        snprintf(n, sizeof n, "ws.enc.raw%d", i); rc = dev_alloc(h, n, (size_t)B * r * r * c, false, &raw); if (rc) return rc;
        snprintf(n, sizeof n, "ws.enc.mean%d", i); rc = dev_alloc(h, n, (size_t)B * c, false, &mean); if (rc) return rc;
        snprintf(n, sizeof n, "ws.enc.std%d", i); rc = dev_alloc(h, n, (size_t)B * c, false, &stdv); if (rc) return rc;
        float* zero_bias; rc = dev_alloc(h, "ws.zero_bias", 2048, true, &zero_bias); if (rc) return rc;
        snprintf(n, sizeof n, "enc.ds%d.kernel", i);
        Op cv = conv_op(e_in, e_in.C, need(n), zero_bias, B, r, c, 2, EPI_BIAS, h->enc_forms[i]);
        set_out_dense(cv.conv, raw, r, r, c);
        const bool fused = fuse_moments_into_splitk(cv, B, 1e-3f, mean, stdv);
        h->ops.push_back(cv);
        if (!fused) h->ops.push_back(moments_op(raw, B, r * r, c, 1e-3f, mean, stdv));
        mom_need(B, r * r, c);
        Op na; na.type = OP_NORMACT;
        snprintf(n, sizeof n, "enc.ds%d.in.gamma", i); na.na.gamma = need(n);
        snprintf(n, sizeof n, "enc.ds%d.in.beta", i); na.na.beta = need(n);
        na.na.x = raw; na.na.mean = mean; na.na.stdv = stdv;
        na.na.B = B; na.na.H = r; na.na.W = r; na.na.C = c; na.na.slope = 0.2f;
        if (i < 5) {
            Padded nx;
            snprintf(n, sizeof n, "ws.enc.p%d", i); rc = alloc_padded(h, n, r, c, &nx); if (rc) return rc;
            set_out_padded(na.na, nx);
            na.na.out_split = h->prec == PREC_BF16X3 ? OUT_BF16X3 : OUT_F32;
            e_in = nx;
        } else {
            rc = dev_alloc(h, "ws.enc.flat", (size_t)B * r * r * c, false, &flat); if (rc) return rc;
            set_out_dense(na.na, flat, r, r, c);
        }
        na.bytes = 2.0 * B * r * r * c * 4;
        h->ops.push_back(na);
    }
    // Dense mean | variance (networks.py:32-33), then the sampler (sampling.py:16) or mean+variance (model.py:267)
    const int K = rlast * rlast * 512;
    float* mv; rc = dev_alloc(h, "ws.enc.mv", (size_t)B * 2 * L, false, &mv); if (rc) return rc;
    rc = dev_alloc(h, "ws.z", (size_t)B * L, false, &h->z); if (rc) return rc;
    size_t dense_part = dense_partial_floats(B, K, 2 * L);
    {
        Op op; op.type = OP_DENSE;
        op.dense = {flat, need("enc.heads.kernel"), need("enc.heads.bias"), mv, B, K, 2 * L};
        op.flops = 2.0 * B * K * 2.0 * L; op.bytes = (double)K * 2 * L * 4;
        h->ops.push_back(op);
        Op lt; lt.type = OP_LATENT; lt.eps_is_input = true;
        lt.lat = {mv, h->z, B, L, h->variant == MSR_GAUGAN ? 1 : 0};
        h->ops.push_back(lt);
    }
    // ---------------- generator (networks.py:37-57) ----------------
    const int sw = S / 64;
    const int N0 = sw * sw * 1024;
    float* x_prev; rc = dev_alloc(h, "ws.gen.x0", (size_t)B * N0, false, &x_prev); if (rc) return rc;
    dense_part = std::max(dense_part, dense_partial_floats(B, L, N0));
    {
        Op op; op.type = OP_DENSE;
        op.dense = {h->z, need("gen.dense.kernel"), need("gen.dense.bias"), x_prev, B, L, N0};
        op.flops = 2.0 * B * L * (double)N0; op.bytes = (double)L * N0 * 4;
        h->ops.push_back(op);
    }
    float *st_mean, *st_std;   // batch moments of the block input
    rc = dev_alloc(h, "ws.gen.mean_in0", 1024, false, &st_mean); if (rc) return rc;
    rc = dev_alloc(h, "ws.gen.std_in0", 1024, false, &st_std); if (rc) return rc;
    h->ops.push_back(moments_op(x_prev, 1, B * sw * sw, 1024, 1e-5f, st_mean, st_std));
    mom_need(1, B * sw * sw, 1024);

    int cin = 1024, r_prev = sw;
    for (int i = 1; i <= 6; ++i) {
        const int f = kGenFilters[i - 1];
        const int r = sw << (i - 1);
        const int shift = i > 1 ? 1 : 0;   // block input = UpSampling2D(previous output), folded into the index
        const bool learned = f != cin;
        float *x1, *skip = nullptr, *outb, *m1, *s1, *mo = nullptr, *so = nullptr;
        snprintf(n, sizeof n, "ws.gen.rb%d.x1", i); rc = dev_alloc(h, n, (size_t)B * r * r * f, false, &x1); if (rc) return rc;
        // fused head: the last block's output exists only as the head's partial sums (32 floats per pixel instead of 128)
        const bool to_head = i == 6 && head_fused_form(h);
        if (to_head) { rc = dev_alloc(h, "ws.gen.head.partial", (size_t)B * r * r * 32, false, &outb); if (rc) return rc; }
        else { snprintf(n, sizeof n, "ws.gen.rb%d.out", i); rc = dev_alloc(h, n, (size_t)B * r * r * f, false, &outb); if (rc) return rc; }
        snprintf(n, sizeof n, "ws.gen.rb%d.mean1", i); rc = dev_alloc(h, n, f, false, &m1); if (rc) return rc;
        snprintf(n, sizeof n, "ws.gen.rb%d.std1", i); rc = dev_alloc(h, n, f, false, &s1); if (rc) return rc;
        if (!to_head) {   // under the fused head nothing computes or reads the last block's output moments: no buffer either
            snprintf(n, sizeof n, "ws.gen.rb%d.meano", i); rc = dev_alloc(h, n, f, false, &mo); if (rc) return rc;
            snprintf(n, sizeof n, "ws.gen.rb%d.stdo", i); rc = dev_alloc(h, n, f, false, &so); if (rc) return rc;
        }
        if (learned) { snprintf(n, sizeof n, "ws.gen.rb%d.skip", i); rc = dev_alloc(h, n, (size_t)B * r * r * f, false, &skip); if (rc) return rc; }

        // one SPADE layer + its consumer conv:  a = lrelu(SPADE(x)) ; y = conv_j(a), both in the forms of the handle's table
        auto spade_then_conv = [&](int j, const float* x, int rx, int xshift, int C, const float* mean, const float* stdv,
                                   float* y, int epi, const float* res, int res_r, int res_shift, bool want_stats) -> int {
            const SpadeForm& sf = h->spade_forms[i][j];
            char k[160];
            // the per-channel scales that go with the fp8 / f16c weight images
            auto wexp = [&](const char* key, const ConvForm& cf) -> const int* {
                if (cf.img != IMG_FP8 && cf.img != IMG_F16C) return nullptr;
                return reinterpret_cast<const int*>(need(std::string(key) + ".wexp"));
            };
            Padded hb, ab;
            int rc2;
            snprintf(k, sizeof k, "ws.gen.rb%d.a%d", i, j);
            // bf8 bytes: one per channel, in slots of four; aslots pads them to the fp8 conv's K
            rc2 = alloc_padded(h, k, r, sf.aslots, &ab, sf.a_split == OUT_BF8 ? C / 4 : sf.aslots); if (rc2) return rc2;
            if (sf.ranges > 0) {
                // conv_gb_resident: the embedding never exists in HBM (no mask-embedding launch, no h buffer); one launch
                // does resize + embedding + gamma|beta conv + SPADE epilogue and writes the consumer's f16c image
                Op g; g.type = OP_GBR; g.src_is_input = true; g.gbr_ranges = sf.ranges;
                GbrParams& q = g.gbr;
                snprintf(k, sizeof k, "gen.rb%d.spade_%d.conv.kernel", i, j); q.we = need(k);
                snprintf(k, sizeof k, "gen.rb%d.spade_%d.conv.kernel.e16", i, j); q.we16 = need(k);
                snprintf(k, sizeof k, "gen.rb%d.spade_%d.conv.bias", i, j); q.be = need(k);
                q.S = S; q.f = S / r; q.o = (S / r) / 2;
                snprintf(k, sizeof k, "gen.rb%d.spade_%d.gb.kernel", i, j); q.wt = need(k);
                snprintf(k, sizeof k, "gen.rb%d.spade_%d.gb.bias", i, j); q.bias = need(k);
                set_aux_dense(q, x, rx, C, xshift);
                q.mean = mean; q.stdv = stdv;
                set_out_padded(q, ab);
                q.out_split = sf.a_split; q.slope = 0.2f;
                q.B = B; q.r = r; q.N = 2 * C;
                q.no_cross = sf.gb.no_cross;
                g.flops = 2.0 * B * r * r * 128.0 * (2 * C) * 9 + 2.0 * B * r * r * 18.0 * 128;
                h->ops.push_back(g);
            } else {
                snprintf(k, sizeof k, "ws.gen.rb%d.h%d", i, j);
                rc2 = alloc_padded(h, k, r, sf.hslots, &hb, sf.h_split == OUT_BF8 ? 128 / 4 : sf.hslots); if (rc2) return rc2;
                Op em; em.type = OP_SMALLCIN; em.src_is_input = true;
                SmallCinParams& p = em.sc;
                snprintf(k, sizeof k, "gen.rb%d.spade_%d.conv.kernel", i, j); p.w = need(k);
                snprintf(k, sizeof k, "gen.rb%d.spade_%d.conv.bias", i, j); p.bias = need(k);
                p.B = B; p.S = S; p.Hout = r; p.Cout = 128;
                p.ay = 1; p.cy = -1; p.lim = r; p.f = S / r; p.o = (S / r) / 2;
                set_out_padded(p, hb);
                p.act = 1; p.slope = 0.f;
                p.out_split = sf.h_split;
                em.flops = 2.0 * B * r * r * 18.0 * 128;
                em.on_aux = true;
                em.aux_group = i <= 4 ? 0 : 1;        // rb1-4 embeds are small and done early; rb5-6 carry the bytes
                if (hipEventCreateWithFlags(&em.done, hipEventDisableTiming) != hipSuccess)
                    return fail(h, MSR_ERR_DEVICE, "hipEventCreate failed");
                h->ops.push_back(em);
                snprintf(k, sizeof k, "gen.rb%d.spade_%d.gb.bias", i, j); const float* gbb = need(k);
                snprintf(k, sizeof k, "gen.rb%d.spade_%d.gb.kernel", i, j);
                Op gb = conv_op(hb, 128, need(k), gbb, B, r, 2 * C, 1, EPI_SPADE, sf.gb);
                gb.conv.wexp = wexp(k, sf.gb);
                gb.conv.out_split = sf.a_split;
                set_out_padded(gb.conv, ab);
                set_aux_dense(gb.conv, x, rx, C, xshift);
                gb.conv.mean = mean; gb.conv.stdv = stdv;
                gb.wait = em.done;
                gb.aux_group = em.aux_group;
                h->ops.push_back(gb);
            }
            snprintf(k, sizeof k, "gen.rb%d.conv_%d.bias", i, j); const float* cb = need(k);
            snprintf(k, sizeof k, "gen.rb%d.conv_%d.kernel", i, j);
            Op cv = conv_op(ab, C, need(k), cb, B, r, f, 1, epi, sf.cv);
            cv.conv.wexp = wexp(k, sf.cv);
            if (epi == EPI_RES_HEAD) { set_out_dense(cv.conv, y, r, r, 32); cv.conv.mean = need("gen.head.wfrag"); }
            else set_out_dense(cv.conv, y, r, r, f);
            if (epi == EPI_RES || epi == EPI_RES_HEAD) set_aux_dense(cv.conv, res, res_r, f, res_shift);
            // fused output moments (the tensor feeds a SPADE layer) unless the layer runs split-K
            if (want_stats && cv.conv.ksplit == 1) cv.stat_slabs = conv_stat_slabs(cv.conv, cv.tile);
            h->ops.push_back(cv);
            return MSR_OK;
        };
        // moments of a conv output: finalize the conv's own slabs if it emitted them, else read the tensor
        auto push_moments = [&](const float* x, int P, int C, float* mean, float* stdv) {
            Op& last = h->ops.back();
            if (fuse_moments_into_splitk(last, 1, 1e-5f, mean, stdv)) {
                mom_need(1, P, C);
            } else if (last.type == OP_CONV && last.stat_slabs > 0) {
                Op op; op.type = OP_MOMENTS_SLABS;
                op.mom = {nullptr, 1, last.stat_slabs, C, 1e-5f, mean, stdv};
                h->ops.push_back(op);
            } else {
                h->ops.push_back(moments_op(x, 1, P, C, 1e-5f, mean, stdv));
                mom_need(1, P, C);
            }
        };
        // x1 = conv_1(lrelu(spade_1(x)))                                   blocks.py:29-30
        rc = spade_then_conv(1, x_prev, r_prev, shift, cin, st_mean, st_std, x1, EPI_BIAS, nullptr, 0, 0, true); if (rc) return rc;
        push_moments(x1, B * r * r, f, m1, s1);
        if (learned) {
            // skip = conv_3(lrelu(spade_3(x)))                             blocks.py:33-34
            rc = spade_then_conv(3, x_prev, r_prev, shift, cin, st_mean, st_std, skip, EPI_BIAS, nullptr, 0, 0, false); if (rc) return rc;
            // out = skip + conv_2(lrelu(spade_2(x1)))                      blocks.py:31-32,38
            rc = spade_then_conv(2, x1, r, 0, f, m1, s1, outb, to_head ? EPI_RES_HEAD : EPI_RES, skip, r, 0, !to_head); if (rc) return rc;
        } else {
            // out = x + conv_2(lrelu(spade_2(x1))), x read through the folded up-sample
            rc = spade_then_conv(2, x1, r, 0, f, m1, s1, outb, to_head ? EPI_RES_HEAD : EPI_RES, x_prev, r_prev, shift, !to_head);
            if (rc) return rc;
        }
        if (to_head) {     // nothing reads the block output or its moments: the gather finishes the head from the partial sums
            Op hg; hg.type = OP_HEAD_GATHER; hg.out_is_output = true;
            hg.hg = {outb, h->host_small["gen.head.bias"][0], B, r};
            hg.flops = 2.0 * B * S * S * 16.0 * 128;      // the head's algorithmic count (its products ran in the conv's epilogue)
            hg.bytes = (double)B * r * r * 32 * 4;
            h->ops.push_back(hg);
            break;
        }
        // moments of the block output == moments of its nearest-2x up-sample (every value is repeated 4x)
        push_moments(outb, B * r * r, f, mo, so);
        x_prev = outb; r_prev = r; cin = f; st_mean = mo; st_std = so;
    }
    if (!head_fused_form(h)) {
        Op hd; hd.type = OP_HEAD; hd.out_is_output = true;
        hd.head = {x_prev, need("gen.head.weff"), h->host_small["gen.head.bias"][0], B, r_prev, 128, 0.2f, 0, 0, 0};
        hd.flops = 2.0 * B * S * S * 16.0 * 128;
        h->ops.push_back(hd);
    }
    // A cross-stream wait stalls the main stream for ~16 us whether or not the event has fired, so the aux stream
    // signals once per group (after the group's last mask-embedding conv; the stream is in order) and only the
    // group's first consumer waits: two groups, i.e. two waits per call.
    for (int grp = 0; grp < 2; ++grp) {
        int last_aux = -1, first_wait = -1;
        for (size_t k = 0; k < h->ops.size(); ++k) {
            if (h->ops[k].aux_group != grp) continue;
            if (h->ops[k].on_aux) last_aux = (int)k;
            else if (first_wait < 0) first_wait = (int)k;
        }
        if (last_aux < 0) continue;
        for (size_t k = 0; k < h->ops.size(); ++k) {
            Op& op = h->ops[k];
            if (op.aux_group != grp) continue;
            if (op.on_aux && (int)k != last_aux) { hipEventDestroy(op.done); op.done = nullptr; }
            if (!op.on_aux) op.wait = (int)k == first_wait ? h->ops[last_aux].done : nullptr;
        }
    }
    mom_doubles = std::max<size_t>(mom_doubles, (size_t)128 * 3 * 1024);  // also the slab-group scratch
    HIPCHK(h, hipMalloc(&h->mom_partial, std::max<size_t>(mom_doubles, 16) * sizeof(double)));
    HIPCHK(h, hipMalloc(&h->dense_partial, std::max<size_t>(dense_part, 16) * sizeof(float)));
    h->mom_partial_bytes = mom_doubles * sizeof(double);
    h->dense_partial_bytes = dense_part * sizeof(float);
    h->total_bytes += h->mom_partial_bytes + h->dense_partial_bytes;
    return MSR_OK;
}

static int plan_pix2pix(msr_handle* h) {
    const int B = h->B;
    char n[128];
    int rc;
    auto fold_bn = [&](const std::string& prefix, int C, float** scale, float** shift) -> int {
        const auto& g = h->host_small[prefix + ".gamma"];
        const auto& b = h->host_small[prefix + ".beta"];
        const auto& m = h->host_small[prefix + ".moving_mean"];
        const auto& v = h->host_small[prefix + ".moving_variance"];
        std::vector<float> sc(C), sh(C);
        for (int c = 0; c < C; ++c) {
            sc[c] = g[c] / std::sqrt(v[c] + 1e-3f);   // keras BatchNormalization epsilon
            sh[c] = b[c] - m[c] * sc[c];
        }
        int r2 = upload(h, prefix + ".scale", sc.data(), C); if (r2) return r2;
        r2 = upload(h, prefix + ".shift", sh.data(), C); if (r2) return r2;
        *scale = D(h, prefix + ".scale"); *shift = D(h, prefix + ".shift");
        return MSR_OK;
    };
    // Activations live in zero-bordered concat buffers cat_i = [up_i | down_(8-i)] (pix2pix.py:99-104 concatenates
    // [x, skip]): a down block writes its half once, the next down block reads it as a channel slice
    // (in_px = total channels) and the up path reads the whole pixel.  No concat copy exists.
    Padded cat[8];           // cat[i], i = 1..7, at resolution 2^i
    Padded d8;               // the 1x1 bottleneck
    for (int i = 1; i <= 7; ++i) {
        const int cu = kP2PUp[i - 1], cd = kP2PDown[6 - (i - 1)];
        snprintf(n, sizeof n, "ws.p2p.cat%d", i);
        rc = alloc_padded(h, n, 1 << i, cu + cd, &cat[i]); if (rc) return rc;
    }
    rc = alloc_padded(h, "ws.p2p.down8", 1, 512, &d8); if (rc) return rc;
    auto igemm = [&](const float* in, int in_px, int in_py, int in_pb, int cin, const float* wt, const float* scale,
                     const float* shift, int rout, int N, int K, int stride, int act, float slope) {
        Op op; op.type = OP_CONV; op.epi = EPI_AFFINE;
        ConvParams& c = op.conv;
        c.in = in; c.wt = wt; c.bias = shift; c.scale = scale; c.act = act; c.slope = slope;
        c.B = B; c.Hout = rout; c.Wout = rout; c.Cin = cin; c.N = N; c.KH = K; c.KW = K; c.stride = stride;
        c.in_px = in_px; c.in_py = in_py; c.in_pb = in_pb;
        const ConvForm f = conv_form(B, rout, N, stride, EPI_AFFINE, PREC_F32, cin, K * K);
        c.prec = f.prec; c.ksplit = f.ksplit;
        op.tile = f.tile; op.kernel = f.kernel;
        op.flops = 2.0 * B * rout * rout * (double)cin * N * K * K;
        return op;
    };
    // ---- down1: 2 -> 64 channels, no BatchNormalization (pix2pix.py:27), on the direct kernel ----
    {
        const Padded& o = cat[7];
        Op op; op.type = OP_DIRECT; op.src_is_input = true;
        DirectConvParams& p = op.dc;
        p.in0 = nullptr; p.c0 = 2; p.in1 = nullptr; p.c1 = 0;
        p.in_px = 2; p.in_py = 256 * 2; p.in_pb = 256 * 256 * 2;
        p.w = D(h, "p2p.down1.kernel"); p.scale = p.shift = nullptr;
        p.out = o.base + o.interior() + kP2PUp[6]; p.out_px = o.C; p.out_py = o.py(); p.out_pb = o.pb();
        p.B = B; p.Hin = 256; p.Win = 256; p.Hout = 128; p.Wout = 128; p.Cout = 64;
        p.KH = 4; p.KW = 4; p.stride = 2; p.pad = 1; p.transposed = 0;
        p.act = 2; p.slope = 0.3f;   // keras LeakyReLU() default alpha (pix2pix.py:72)
        op.flops = 2.0 * B * 128 * 128 * 16.0 * 2 * 64;
        h->ops.push_back(op);
    }
    // ---- down2..8: 4x4 stride-2 implicit GEMM; the padded border is the 'same' padding (1 before, 1 after) ----
    for (int i = 2; i <= 8; ++i) {
        const int cin = kP2PDown[i - 2], c = kP2PDown[i - 1];
        const Padded& src = cat[8 - (i - 1)];
        const int src_off = kP2PUp[8 - (i - 1) - 1];          // the skip half starts after the up half
        const int rout = 256 >> i;
        snprintf(n, sizeof n, "p2p.down%d.bn", i);
        float *sc, *sh; rc = fold_bn(n, c, &sc, &sh); if (rc) return rc;
        snprintf(n, sizeof n, "p2p.down%d.kernel", i);
        Op op = igemm(src.base + src_off, src.C, src.py(), src.pb(), cin, D(h, n), sc, sh, rout, c, 4, 2, 2, 0.3f);
        if (i < 8) {
            const Padded& o = cat[8 - i];
            set_out_padded(op.conv, o);
            op.conv.out_off += kP2PUp[8 - i - 1];
        } else {
            set_out_padded(op.conv, d8);
        }
        h->ops.push_back(op);
    }
    // ---- up1..7: Conv2DTranspose + BatchNormalization (+ Dropout, identity at inference) + ReLU
    //      (pix2pix.py:76-94) as four parity sub-convolutions writing interleaved pixels of cat_i's up half ----
    for (int i = 1; i <= 7; ++i) {
        const Padded& src = i == 1 ? d8 : cat[i - 1];
        const Padded& o = cat[i];
        const int c = kP2PUp[i - 1], r = src.r;
        snprintf(n, sizeof n, "p2p.up%d.bn", i);
        float *sc, *sh; rc = fold_bn(n, c, &sc, &sh); if (rc) return rc;
        snprintf(n, sizeof n, "p2p.up%d.kernel", i);
        const float* w = D(h, n);
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                Op op = igemm(src.base + py * src.py() + px * src.C, src.C, src.py(), src.pb(), src.C,
                              w + (size_t)(py * 2 + px) * 4 * c * src.C, sc, sh, r, c, 2, 1, 1, 0.f);
                ConvParams& cp = op.conv;
                cp.out = o.base; cp.out_px = 2 * o.C; cp.out_py = 2 * o.py(); cp.out_pb = o.pb();
                cp.out_off = o.interior() + py * o.py() + px * o.C;
                h->ops.push_back(op);
            }
    }
    // ---- last: Conv2DTranspose(1, 4, 2, 'same', tanh) (pix2pix.py:53-57) = per-parity 2x2 taps on the head kernel ----
    {
        const Padded& src = cat[7];
        Op op; op.type = OP_HEAD;
        op.head = {src.base + src.interior(), D(h, "p2p.last.weff"), h->host_small["p2p.last.bias"][0], B, 128, src.C,
                   1.0f, 1, src.py(), src.pb()};
        op.flops = 2.0 * B * 128 * 128 * 16.0 * src.C;
        h->ops.push_back(op);
    }
    return MSR_OK;
}

void drop_graphs(msr_handle* h) {
    for (auto& g : h->graphs) {
        if (g.exec) hipGraphExecDestroy(g.exec);
        if (g.graph) hipGraphDestroy(g.graph);
    }
    h->graphs.clear();
    h->seen_once.clear();
}

int ensure_conv_partial(msr_handle* h, size_t floats) {
    if (floats <= h->conv_partial_floats) return MSR_OK;
    if (!h->graphs.empty()) {      // instantiated graphs hold the old pointer: a replay would write split-K partials into freed memory
        HIPCHK(h, hipDeviceSynchronize());
        drop_graphs(h);
    }
    if (h->conv_partial) HIPCHK(h, hipFree(h->conv_partial));
    h->conv_partial = nullptr;
    HIPCHK(h, hipMalloc(&h->conv_partial, floats * sizeof(float)));
    h->total_bytes += (floats - h->conv_partial_floats) * sizeof(float);
    h->conv_partial_floats = floats;
    return MSR_OK;
}

// The tensors msr_range_scan reads: every planned activation image written in a format whose pieces have a finite range
// (OUT_F16X2 .. OUT_F16C6), once each, in plan order; and the gbr ops, whose embedding is bounded on the host instead.
static void build_range_plan(msr_handle* h) {
    h->range_plan.clear();
    h->range_embeds.clear();
    h->range_table_stale = true;
    auto tensor_of = [&](const void* ptr) -> std::string {
        const char* nm = name_of(h, ptr);
        return nm ? nm : "";
    };
    auto add = [&](int producer, const float* out, int out_off, int split, int B, int r, int C, int px_floats) {
        if (split < OUT_F16X2 || split > OUT_F16C6 || !out || C % 32) return;
        const std::string nm = tensor_of(out);
        if (nm.empty() || nm.size() >= 48) return;
        if (split != OUT_BF8 && px_floats != C) return;                       // chunk formats: one float slot per channel
        for (const auto& e : h->range_plan) if (e.tensor == nm) return;
        RangeScanItem it{out, split, B, r, C, px_floats * 4, out_off != 0, (int)h->range_plan.size()};
        h->range_plan.push_back({nm, producer, it});
    };
    for (size_t k = 0; k < h->ops.size(); ++k) {
        const Op& op = h->ops[k];
        if (op.type == OP_CONV) {
            const ConvParams& c = op.conv;
            add((int)k, c.out, c.out_off, c.out_split, c.B, c.Hout, op.epi == EPI_SPADE ? c.N / 2 : c.N, c.out_px);
        } else if (op.type == OP_GBR) {
            const GbrParams& q = op.gbr;
            add((int)k, q.out, q.out_off, q.out_split, q.B, q.r, q.N / 2, q.out_px);
            h->range_embeds.push_back({tensor_of(q.we), (int)k});
        } else if (op.type == OP_SMALLCIN) {
            const SmallCinParams& p = op.sc;
            add((int)k, p.out, p.out_off, p.out_split, p.B, p.Hout, p.Cout, p.out_px);
        }
    }
}

int ensure_plan(msr_handle* h) {
    if (h->planned) return MSR_OK;
    for (auto& s : h->specs)
        if (!s.loaded) return fail(h, MSR_ERR_STATE, "weight '%s' has not been loaded", s.name.c_str());
    for (auto& op : h->ops)
        if (op.done) hipEventDestroy(op.done);
    h->ops.clear();
    drop_graphs(h);                       // they hold the old plan's pointers
    if (!h->aux) {
        HIPCHK(h, hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking));   // (stream priority, low or high, changes nothing: measured)
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        // First use now: HIP binds a stream to a hardware queue when it is first used, in order, and queues whose ids
        // are equal modulo 4 share a dispatch pipe (profiles/r02_raster_queue_pairing.txt).  Callers that pipeline two
        // handles plan them back to back (Generator.prepare) so that their four busy streams land on four pipes.
        float* touch = nullptr;
        if (dev_alloc(h, "ws.aux_touch", 4, false, &touch) == MSR_OK) HIPCHK(h, hipMemsetAsync(touch, 0, 16, h->aux));
    }
    if (h->mom_partial) { hipFree(h->mom_partial); h->mom_partial = nullptr; }
    if (h->dense_partial) { hipFree(h->dense_partial); h->dense_partial = nullptr; }
    h->total_bytes -= h->mom_partial_bytes + h->dense_partial_bytes;     // a re-plan allocates and counts them again
    h->mom_partial_bytes = h->dense_partial_bytes = 0;
    int rc = h->variant == MSR_PIX2PIX ? plan_pix2pix(h) : plan_spade(h);
    if (rc) return rc;
    h->fwd_flops = 0;
    h->gate_op = -1;
    for (size_t k = 0; k < h->ops.size(); ++k)
        if (h->ops[k].type == OP_GBR ||
            (h->ops[k].type == OP_CONV && h->ops[k].tile == TILE_256x128_PP && h->ops[k].conv.ksplit == 1)) {
            h->gate_op = (int)k;     // first layer that fills the chip with persistent ping-pong tiles
            break;
        }
    size_t need = 0, stat_need = 0;
    for (auto& op : h->ops) {
        h->fwd_flops += op.flops;
        if (op.type == OP_CONV && op.conv.ksplit > 1)
            need = std::max(need, (size_t)op.conv.ksplit * op.conv.B * op.conv.Hout * op.conv.Wout * op.conv.N);
        if (op.type == OP_CONV && op.stat_slabs > 0)
            stat_need = std::max(stat_need, (size_t)op.stat_slabs * 3 * op.conv.N);
    }
    { int rc2 = ensure_conv_partial(h, need); if (rc2) return rc2; }
    if (stat_need > h->stat_ws_floats) {
        if (h->stat_ws) HIPCHK(h, hipFree(h->stat_ws));
        h->stat_ws = nullptr;
        HIPCHK(h, hipMalloc(&h->stat_ws, stat_need * sizeof(float)));
        h->total_bytes += (stat_need - h->stat_ws_floats) * sizeof(float);
        h->stat_ws_floats = stat_need;
    }
    HIPCHK(h, hipDeviceSynchronize());
    build_range_plan(h);
    h->planned = true;
    return MSR_OK;
}

}  // namespace msr

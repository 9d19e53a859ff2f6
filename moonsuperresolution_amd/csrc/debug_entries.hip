// debug_entries.hip — what a test or a tool reads back from a handle: device tensors by name, the planned forms as text
// (msr_debug_*), the activation-range scan (msr_range_*) and the device-memory total.
#include "host.h"

using namespace msr;

void msr::range_fill(msr_range_stat* o, const std::string& tensor, int format, int producer, const RangeScanRecord& r) {
    std::memset(o, 0, sizeof *o);
    snprintf(o->tensor, sizeof o->tensor, "%s", tensor.c_str());
    o->format = format;
    o->producer = producer;
    std::memcpy(&o->max_abs, &r.max_abs_bits, sizeof(float));
    o->n_total = (int64_t)r.n_total;
    o->n_cross_clipped = (int64_t)r.n_cross_clipped;
    o->n_clamped = (int64_t)r.n_clamped;
    o->n_nonfinite = (int64_t)r.n_nonfinite;
}

static const char* const kImg[] = {"F32", "BF16", "BF16_FRAG", "F16", "FP8", "F16C", "F16C6", "GBR"};       // WeightImage
static const char* const kKernel[] = {"generic", "bvgpr", "halo", "halo16", "pp", "sw"};                     // ConvKernel

extern "C" {

int msr_debug_tensor(msr_handle* h, const char* name, float* host_out, int64_t count) {
    if (!h || !name || !host_out) return MSR_ERR_INVALID;
    auto it = h->dev.find(name);
    if (it == h->dev.end() && !std::strcmp(name, "ws.gen.rb6.out") && head_fused_form(h))
        return fail(h, MSR_ERR_INVALID, "ws.gen.rb6.out does not exist under MSR_FLAG_FUSED_HEAD: gen.rb6.conv_2 writes the head's "
                    "partial sums ws.gen.head.partial [B, r, r, 32] instead of its output");
    if (it == h->dev.end()) return fail(h, MSR_ERR_INVALID, "no tensor named '%s'", name);
    if (count < 0 || (size_t)count * sizeof(float) > h->dev_bytes[name])
        return fail(h, MSR_ERR_INVALID, "%s holds %zu floats, %lld requested", name, h->dev_bytes[name] / sizeof(float),
                    (long long)count);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(host_out, it->second, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
    return MSR_OK;
}

int msr_debug_moment_forms(msr_handle* h, char* out, int64_t cap) {
    if (!h || !out || cap < 1) return MSR_ERR_INVALID;
    // one line "<mean tensor> <form>" per planned moments site, in plan order.  Forms: A moments kernels over the tensor,
    // B split-K epilogue, E1 / E2 one- / two-stage slab finalize after the slabs of the conv_igemm epilogue (/C) or of
    // the ping-pong / stream kernels (/D)
    auto tensor_of = [&](const float* ptr) -> std::string {
        const char* nm = name_of(h, ptr);
        return nm ? nm : "?";
    };
    std::string txt;
    for (size_t i = 0; i < h->ops.size(); ++i) {
        const Op& op = h->ops[i];
        if (op.type == OP_MOMENTS) {
            txt += tensor_of(op.mom.mean) + " A\n";
        } else if (op.type == OP_CONV && op.conv.mom_mean) {
            txt += tensor_of(op.conv.mom_mean) + " B\n";
        } else if (op.type == OP_MOMENTS_SLABS && i > 0) {
            const bool two = op.mom.P >= 512;
            txt += tensor_of(op.mom.mean) + (two ? " E2/" : " E1/") + (h->ops[i - 1].tile == TILE_256x128_PP ? "D\n" : "C\n");
        }
    }
    if ((int64_t)txt.size() + 1 > cap) return fail(h, MSR_ERR_INVALID, "msr_debug_moment_forms: %zu bytes needed", txt.size() + 1);
    memcpy(out, txt.c_str(), txt.size() + 1);
    return MSR_OK;
}

int msr_debug_conv_forms(msr_handle* h, char* out, int64_t cap) {
    if (!h || !out || cap < 1) return MSR_ERR_INVALID;
    // one line of "key=value" words per planned op, in plan order (moonsr.h).  Tensors are named by the handle's reverse
    // lookup; a pointer into a buffer (a stride-2 conv reads from the interior of its padded input) names the buffer.
    auto tensor_of = [&](const void* ptr) -> std::string {
        if (!ptr) return "-";
        const char* nm = name_of(h, ptr);
        return nm ? nm : "?";
    };
    auto img_of = [&](const std::string& key) -> const char* {
        auto it = h->dev_img.find(key);
        return it == h->dev_img.end() ? "?" : kImg[it->second];
    };
    std::string txt;
    char b[1024];
    for (const Op& op : h->ops) {
        switch (op.type) {
            case OP_CONV: {
                const ConvParams& c = op.conv;
                const std::string wt = tensor_of(c.wt);
                snprintf(b, sizeof b, "kind=conv in=%s wt=%s wexp=%s bias=%s aux=%s mean=%s std=%s out=%s prec=%d kernel=%s tile=%d ksplit=%d "
                         "wt_frag=%d no_cross=%d epi=%d out_split=%d ranges=0 img=%s B=%d r=%d cin=%d N=%d stride=%d aux_shift=%d "
                         "stat_slabs=%d mom=%s\n", tensor_of(c.in).c_str(), wt.c_str(), tensor_of(c.wexp).c_str(),
                         tensor_of(c.bias).c_str(), tensor_of(c.aux).c_str(), tensor_of(c.mean).c_str(), tensor_of(c.stdv).c_str(),
                         tensor_of(c.out).c_str(), c.prec, op.kernel >= 0 ? kKernel[op.kernel] : "none", op.tile, c.ksplit, c.wt_frag, c.no_cross, op.epi, c.out_split,
                         img_of(wt), c.B, c.Hout, c.Cin, c.N, c.stride, c.aux_shift, op.stat_slabs, tensor_of(c.mom_mean).c_str());
                break;
            }
            case OP_GBR: {
                const GbrParams& q = op.gbr;
                const std::string wt = tensor_of(q.wt);
                snprintf(b, sizeof b, "kind=gbr in=input wt=%s embed=%s embed16=%s embed_bias=%s bias=%s aux=%s mean=%s std=%s out=%s "
                         "prec=%d kernel=gbr tile=%d ksplit=1 wt_frag=0 no_cross=%d epi=%d out_split=%d ranges=%d img=%s B=%d r=%d cin=128 N=%d "
                         "stride=1 aux_shift=%d\n", wt.c_str(), tensor_of(q.we).c_str(), tensor_of(q.we16).c_str(),
                         tensor_of(q.be).c_str(), tensor_of(q.bias).c_str(), tensor_of(q.aux).c_str(), tensor_of(q.mean).c_str(),
                         tensor_of(q.stdv).c_str(), tensor_of(q.out).c_str(), (int)PREC_F16C6, (int)TILE_256x128_PP, q.no_cross,
                         (int)EPI_SPADE, q.out_split, op.gbr_ranges, img_of(wt), q.B, q.r, q.N, q.aux_shift);
                break;
            }
            case OP_SMALLCIN: {
                const SmallCinParams& p = op.sc;
                snprintf(b, sizeof b, "kind=smallcin in=input wt=%s bias=%s out=%s out_split=%d B=%d r=%d N=%d stride=%d act=%d "
                         "on_aux=%d\n", tensor_of(p.w).c_str(), tensor_of(p.bias).c_str(), tensor_of(p.out).c_str(), p.out_split, p.B,
                         p.Hout, p.Cout, p.ay, p.act, op.on_aux ? 1 : 0);
                break;
            }
            case OP_MOMENTS:
            case OP_MOMENTS_SLABS:
                snprintf(b, sizeof b, "kind=%s in=%s mean=%s std=%s\n", op.type == OP_MOMENTS ? "moments" : "moments_slabs",
                         tensor_of(op.mom.x).c_str(), tensor_of(op.mom.mean).c_str(), tensor_of(op.mom.stdv).c_str());
                break;
            case OP_NORMACT:
                snprintf(b, sizeof b, "kind=norm_act in=%s mean=%s std=%s gamma=%s beta=%s out=%s out_split=%d B=%d r=%d N=%d\n",
                         tensor_of(op.na.x).c_str(), tensor_of(op.na.mean).c_str(), tensor_of(op.na.stdv).c_str(),
                         tensor_of(op.na.gamma).c_str(), tensor_of(op.na.beta).c_str(), tensor_of(op.na.out).c_str(), op.na.out_split,
                         op.na.B, op.na.H, op.na.C);
                break;
            case OP_DENSE:
                snprintf(b, sizeof b, "kind=dense in=%s wt=%s bias=%s out=%s B=%d cin=%d N=%d\n", tensor_of(op.dense.x).c_str(),
                         tensor_of(op.dense.W).c_str(), tensor_of(op.dense.bias).c_str(), tensor_of(op.dense.y).c_str(), op.dense.B,
                         op.dense.K, op.dense.N);
                break;
            case OP_LATENT:
                snprintf(b, sizeof b, "kind=latent in=%s aux=eps out=%s B=%d N=%d sampler=%d\n", tensor_of(op.lat.mv).c_str(),
                         tensor_of(op.lat.z).c_str(), op.lat.B, op.lat.L, op.lat.sampler);
                break;
            case OP_HEAD:
                snprintf(b, sizeof b, "kind=head in=%s wt=%s out=output B=%d r=%d cin=%d tanh=%d\n", tensor_of(op.head.x).c_str(),
                         tensor_of(op.head.weff).c_str(), op.head.B, op.head.r, op.head.C, op.head.tanh_out);
                break;
            case OP_HEAD_GATHER:
                snprintf(b, sizeof b, "kind=head_gather in=%s out=output B=%d r=%d\n", tensor_of(op.hg.partial).c_str(), op.hg.B,
                         op.hg.r);
                break;
            case OP_DIRECT:
                snprintf(b, sizeof b, "kind=direct in=%s wt=%s out=%s B=%d r=%d N=%d\n", op.src_is_input ? "input" : tensor_of(op.dc.in0).c_str(),
                         tensor_of(op.dc.w).c_str(), op.out_is_output ? "output" : tensor_of(op.dc.out).c_str(), op.dc.B, op.dc.Hout,
                         op.dc.Cout);
                break;
        }
        txt += b;
    }
    if ((int64_t)txt.size() + 1 > cap) return fail(h, MSR_ERR_INVALID, "msr_debug_conv_forms: %zu bytes needed", txt.size() + 1);
    memcpy(out, txt.c_str(), txt.size() + 1);
    return MSR_OK;
}

int msr_debug_f16c_kernel(int32_t cin, int32_t epilogue, int32_t out_mode) {
    return conv_kernel_for(PREC_F16C, TILE_256x128_PP, 1, 0, cin, epilogue, epilogue == EPI_SPADE ? out_mode : OUT_F32) == KERNEL_SW;
}

int msr_debug_form_table(const msr_config* cfg, char* out, int64_t cap) {
    if (!cfg || !out || cap < 1) return fail(nullptr, MSR_ERR_INVALID, "msr_debug_form_table: null argument");
    msr_handle h;
    int rc = configure(&h, cfg);
    if (rc) return rc;
    fill_forms(&h);
    std::string txt;
    char b[256];
    auto conv_line = [&](const char* name, const ConvForm& f, bool gbr = false) {
        snprintf(b, sizeof b, "%s prec=%d kernel=%s tile=%d ksplit=%d wt_frag=%d no_cross=%d img=%s\n", name, f.prec,
                 gbr ? "gbr" : f.kernel >= 0 ? kKernel[f.kernel] : "none", f.tile, f.ksplit, f.wt_frag, f.no_cross, kImg[f.img]);
        txt += b;
    };
    char n[96];
    if (h.variant == MSR_PIX2PIX) {      // the conv_form calls of plan_pix2pix
        for (int i = 2; i <= 8; ++i) {
            snprintf(n, sizeof n, "p2p.down%d", i);
            conv_line(n, conv_form(h.B, 256 >> i, kP2PDown[i - 1], 2, EPI_AFFINE, PREC_F32, kP2PDown[i - 2], 16));
        }
        for (int i = 1; i <= 7; ++i) {   // input: the 1 x 1 bottleneck, then the concat buffer [up_(i-1) | down_(9-i)]
            const int cin = i == 1 ? kP2PDown[7] : kP2PUp[i - 2] + kP2PDown[8 - i];
            snprintf(n, sizeof n, "p2p.up%d", i);
            conv_line(n, conv_form(h.B, 1 << (i - 1), kP2PUp[i - 1], 1, EPI_AFFINE, PREC_F32, cin, 4));
        }
    } else {
        for (int i = 2; i <= 5; ++i) {
            snprintf(n, sizeof n, "enc.ds%d", i);
            conv_line(n, h.enc_forms[i]);
        }
        int cin = 1024;
        for (int i = 1; i <= 6; cin = kGenFilters[i - 1], ++i)
            for (int j = 1; j <= (kGenFilters[i - 1] != cin ? 3 : 2); ++j) {
                const SpadeForm& s = h.spade_forms[i][j];
                snprintf(n, sizeof n, "gen.rb%d.spade_%d.gb", i, j);
                conv_line(n, s.gb, s.ranges > 0);
                snprintf(b, sizeof b, "gen.rb%d.spade_%d gbr=%d ranges=%d h_split=%d hslots=%d a_split=%d aslots=%d\n", i, j,
                         s.ranges > 0 ? 1 : 0, s.ranges, s.h_split, s.hslots, s.a_split, s.aslots);
                txt += b;
                snprintf(n, sizeof n, "gen.rb%d.conv_%d", i, j);
                conv_line(n, s.cv);
            }
    }
    txt += head_fused_form(&h) ? "head_fused=1\n" : "head_fused=0\n";
    if ((int64_t)txt.size() + 1 > cap) return fail(nullptr, MSR_ERR_INVALID, "msr_debug_form_table: %zu bytes needed", txt.size() + 1);
    memcpy(out, txt.c_str(), txt.size() + 1);
    return MSR_OK;
}

int msr_range_scan(msr_handle* h, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!h->forward_seen) return fail(h, MSR_ERR_STATE, "msr_range_scan: no msr_forward has run on this handle yet");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = h->range_plan.size();
    h->range_enqueued = true;
    if (n == 0) return MSR_OK;                       // fp32 / bf16x3 plans hold no narrow tensor
    if (!h->range_done) HIPCHK(h, hipEventCreateWithFlags(&h->range_done, hipEventDisableTiming));
    if (h->range_cap < n) {
        // table (device), records (device, pinned host), and a pinned staging copy of the table behind the records
        if (h->range_table_dev) { HIPCHK(h, hipFree(h->range_table_dev)); h->range_table_dev = nullptr; }
        if (h->range_rec_dev) { HIPCHK(h, hipFree(h->range_rec_dev)); h->range_rec_dev = nullptr; }
        if (h->range_rec_host) { HIPCHK(h, hipHostFree(h->range_rec_host)); h->range_rec_host = nullptr; }
        h->total_bytes -= h->range_cap * (sizeof(RangeScanItem) + sizeof(RangeScanRecord));
        h->range_cap = 0;
        HIPCHK(h, hipMalloc(&h->range_table_dev, n * sizeof(RangeScanItem)));
        HIPCHK(h, hipMalloc(&h->range_rec_dev, n * sizeof(RangeScanRecord)));
        HIPCHK(h, hipHostMalloc(&h->range_rec_host, n * (sizeof(RangeScanRecord) + sizeof(RangeScanItem)), hipHostMallocDefault));
        h->range_cap = n;
        h->total_bytes += n * (sizeof(RangeScanItem) + sizeof(RangeScanRecord));
        h->range_table_stale = true;
    }
    int max_rows = 1;
    for (const auto& e : h->range_plan) max_rows = std::max(max_rows, e.item.B * e.item.r);
    if (h->range_table_stale) {
        RangeScanItem* stage = reinterpret_cast<RangeScanItem*>(h->range_rec_host + h->range_cap);
        for (size_t k = 0; k < n; ++k) stage[k] = h->range_plan[k].item;
        HIPCHK(h, hipMemcpyAsync(h->range_table_dev, stage, n * sizeof(RangeScanItem), hipMemcpyHostToDevice, s));
        h->range_table_stale = false;
    }
    HIPCHK(h, hipMemsetAsync(h->range_rec_dev, 0, n * sizeof(RangeScanRecord), s));
    HIPCHK(h, launch_range_scan(h->range_table_dev, (int)n, h->range_rec_dev, max_rows, s));
    HIPCHK(h, hipMemcpyAsync(h->range_rec_host, h->range_rec_dev, n * sizeof(RangeScanRecord), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipEventRecord(h->range_done, s));
    return MSR_OK;
}

int msr_range_read(msr_handle* h, msr_range_stat* out, int32_t cap, int32_t* n) {
    if (!h || !n || cap < 0 || (cap > 0 && !out)) return MSR_ERR_INVALID;
    if (!h->range_enqueued) return fail(h, MSR_ERR_STATE, "msr_range_read: no msr_range_scan was enqueued");
    const size_t cnt = h->range_plan.size();
    if (cnt && h->range_done) HIPCHK(h, hipEventSynchronize(h->range_done));
    *n = (int32_t)cnt;
    for (size_t k = 0; k < cnt && (int32_t)k < cap; ++k) {
        const auto& e = h->range_plan[k];
        range_fill(out + k, e.tensor, e.item.format, e.producer, h->range_rec_host[k]);
    }
    return MSR_OK;
}

int msr_range_embed_bounds(msr_handle* h, msr_range_stat* out, int32_t cap, int32_t* n) {
    if (!h || !n || cap < 0 || (cap > 0 && !out)) return MSR_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = ensure_plan(h);
    if (rc) return rc;
    *n = (int32_t)h->range_embeds.size();
    for (size_t k = 0; k < h->range_embeds.size() && (int32_t)k < cap; ++k) {
        const auto& e = h->range_embeds[k];
        const auto w = h->host_small.find(e.kernel);
        const auto b = h->host_small.find(e.kernel.substr(0, e.kernel.size() - 6) + "bias");
        if (w == h->host_small.end() || b == h->host_small.end() || w->second.size() != 18 * 128 || b->second.size() != 128)
            return fail(h, MSR_ERR_STATE, "msr_range_embed_bounds: no host copy of %s", e.kernel.c_str());
        // HWIO [3, 3, 2, 128]: |embedding_c| <= 0.5 * sum |w[., ., ., c]| + |b_c| for inputs in [-0.5, 0.5]
        double worst = 0.0;
        for (int c = 0; c < 128; ++c) {
            double sum = 0.0;
            for (int t = 0; t < 18; ++t) sum += std::fabs((double)w->second[(size_t)t * 128 + c]);
            worst = std::max(worst, 0.5 * sum + std::fabs((double)b->second[c]));
        }
        RangeScanRecord r{};
        const float bound = (float)worst;
        std::memcpy(&r.max_abs_bits, &bound, sizeof(float));
        range_fill(out + k, e.kernel, MSR_RANGE_FORMAT_EMBED, e.producer, r);
    }
    return MSR_OK;
}

int msr_debug_workspace_list(msr_handle* h, char* out, int64_t cap) {
    if (!h || !out || cap < 1) return MSR_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = ensure_plan(h);
    if (rc) return rc;
    std::string txt;
    char b[256];
    auto line = [&](const std::string& name, const char* kind, size_t bytes, int zeroed, int counted) {
        snprintf(b, sizeof b, "name=%s kind=%s bytes=%zu zeroed=%d counted=%d", name.c_str(), kind, bytes, zeroed, counted);
        txt += b;
    };
    for (const auto& kv : h->dev) {
        const bool ws = kv.first.compare(0, 3, "ws.") == 0;
        const auto z = h->dev_zeroed.find(kv.first);
        line(kv.first, ws ? "ws" : "weight", h->dev_bytes[kv.first], z != h->dev_zeroed.end() && z->second ? 1 : 0, 1);
        const auto p = h->dev_padded.find(kv.first);
        if (p != h->dev_padded.end()) {
            snprintf(b, sizeof b, " r=%d C=%d written=%d", p->second.r, p->second.C, p->second.written);
            txt += b;
        }
        txt += "\n";
    }
    if (h->mom_partial) { line("scratch.mom_partial", "scratch", h->mom_partial_bytes, 0, 1); txt += "\n"; }
    if (h->dense_partial) { line("scratch.dense_partial", "scratch", h->dense_partial_bytes, 0, 1); txt += "\n"; }
    if (h->conv_partial) { line("scratch.conv_partial", "scratch", h->conv_partial_floats * sizeof(float), 0, 1); txt += "\n"; }
    if (h->stat_ws) { line("scratch.stat_ws", "scratch", h->stat_ws_floats * sizeof(float), 0, 1); txt += "\n"; }
    // tables: indices, offsets and constants.  The tiler's two are not part of msr_device_bytes.
    if (h->range_cap) {
        line("table.range_items", "table", h->range_cap * sizeof(RangeScanItem), 0, 1); txt += "\n";
        line("table.range_records", "table", h->range_cap * sizeof(RangeScanRecord), 0, 1); txt += "\n";
    }
    if (h->window) {
        const size_t ws = (size_t)(h->S - 2 * (h->S / 16));
        line("table.blend_window", "table", ws * ws * sizeof(double), 0, 0); txt += "\n";
    }
    if (h->stitch_grid) { line("table.stitch_grid", "table", (size_t)h->stitch_grid_cap * sizeof(int), 0, 0); txt += "\n"; }
    if ((int64_t)txt.size() + 1 > cap) return fail(h, MSR_ERR_INVALID, "msr_debug_workspace_list: %zu bytes needed", txt.size() + 1);
    memcpy(out, txt.c_str(), txt.size() + 1);
    return MSR_OK;
}

int msr_debug_fill_workspace(msr_handle* h, int32_t what, int32_t byte, int64_t* bytes_filled) {
    if (!h || !bytes_filled) return MSR_ERR_INVALID;
    *bytes_filled = 0;
    if (what < 1 || what > 7 || byte < 0 || byte > 255)
        return fail(h, MSR_ERR_INVALID, "msr_debug_fill_workspace: what must be in 1..7 and byte in 0..255, got %d and %d", what, byte);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = ensure_plan(h);                 // a planned handle returns at once: captured graphs stay
    if (rc) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    size_t total = 0;
    // Only activations and partial sums are written here: the keys that begin with "ws." and the four scratch buffers.  Weights,
    // .wexp, the folded scales, ws.zero_bias (zeroed, not padded), the blend window, stitch_grid and the range-scan tables hold
    // constants, indices or offsets and are never touched, so that a stale read shows as a wrong number, never as an address.
    if (what & 1) {
        for (const auto& kv : h->dev) {
            const auto z = h->dev_zeroed.find(kv.first);
            if (kv.first.compare(0, 3, "ws.") != 0 || z == h->dev_zeroed.end() || z->second) continue;
            const size_t n = h->dev_bytes[kv.first];
            if (n) HIPCHK(h, hipMemset(kv.second, byte, n));
            total += n;
        }
        const struct { void* p; size_t n; } scratch[] = {{h->mom_partial, h->mom_partial_bytes},
                                                         {h->dense_partial, h->dense_partial_bytes},
                                                         {h->conv_partial, h->conv_partial_floats * sizeof(float)},
                                                         {h->stat_ws, h->stat_ws_floats * sizeof(float)}};
        for (const auto& s : scratch)
            if (s.p && s.n) { HIPCHK(h, hipMemset(s.p, byte, s.n)); total += s.n; }
    }
    for (const auto& kv : h->dev_padded) {
        const auto it = h->dev.find(kv.first);
        if (it == h->dev.end() || !(what & 6)) continue;
        const size_t r = (size_t)kv.second.r, C = (size_t)kv.second.C, wr = (size_t)kv.second.written, F = sizeof(float);
        const size_t py = (r + 2) * C, pb = (r + 2) * py;
        if (h->dev_bytes[kv.first] != (size_t)h->B * pb * F)
            return fail(h, MSR_ERR_STATE, "msr_debug_fill_workspace: %s is not [%d, %zu, %zu, %zu]", kv.first.c_str(), h->B, r + 2, r + 2, C);
        for (int bi = 0; bi < h->B; ++bi) {
            float* img = it->second + (size_t)bi * pb;
            if (what & 2) {                  // interior pixels, the slots the producer writes
                if (wr == C) {
                    HIPCHK(h, hipMemset2D(img + py + C, py * F, byte, r * C * F, r));
                } else {
                    for (size_t y = 1; y <= r; ++y) HIPCHK(h, hipMemset2D(img + y * py + C, C * F, byte, wr * F, r));
                }
                total += r * r * wr * F;
            }
            if (what & 4) {                  // the border: rows 0 and r + 1, columns 0 and r + 1 of the rows between, every slot
                HIPCHK(h, hipMemset(img, byte, py * F));
                HIPCHK(h, hipMemset(img + (r + 1) * py, byte, py * F));
                HIPCHK(h, hipMemset2D(img + py, py * F, byte, C * F, r));
                HIPCHK(h, hipMemset2D(img + py + (r + 1) * C, py * F, byte, C * F, r));
                total += (2 * py + 2 * r * C) * F;
            }
        }
    }
    HIPCHK(h, hipDeviceSynchronize());
    *bytes_filled = (int64_t)total;
    return MSR_OK;
}

int msr_device_bytes(const msr_handle* h, int64_t* bytes) {
    if (!h || !bytes) return MSR_ERR_INVALID;
    *bytes = (int64_t)h->total_bytes;
    return MSR_OK;
}

}  // extern "C"

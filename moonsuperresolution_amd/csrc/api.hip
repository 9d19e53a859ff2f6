// api.hip — the handle of libmoonsr_hip.so (include/moonsr.h): creation, errors, the device-buffer table, the weight specs
// and the weight loader.  Host logic only; the other host units are listed in host.h, kernels live in the kernel files.
#include "host.h"

#include <cstdarg>
#include <memory>

using namespace msr;

static thread_local std::string g_create_error;

namespace msr {

int fail(msr_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

const char* name_of(const msr_handle* h, const void* ptr) {
    if (!ptr) return nullptr;
    const char* q = static_cast<const char*>(ptr);
    for (const auto& kv : h->dev) {
        const char* b = reinterpret_cast<const char*>(kv.second);
        const auto sz = h->dev_bytes.find(kv.first);
        if (q >= b && q < b + std::max<size_t>(sz == h->dev_bytes.end() ? 0 : sz->second, 16)) return kv.first.c_str();
    }
    return nullptr;
}

int dev_alloc(msr_handle* h, const std::string& key, size_t floats, bool zero, float** out) {
    auto it = h->dev.find(key);
    if (it != h->dev.end()) {
        if (h->dev_bytes[key] != floats * sizeof(float))
            return fail(h, MSR_ERR_STATE, "buffer %s re-allocated with a different size", key.c_str());
        *out = it->second;
        return MSR_OK;
    }
    float* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(floats, 4) * sizeof(float));
    if (e != hipSuccess)
        return fail(h, MSR_ERR_NOMEM, "hipMalloc of %zu bytes for %s failed: %s", floats * sizeof(float), key.c_str(),
                    hipGetErrorString(e));
    if (zero) {
        e = hipMemset(p, 0, std::max<size_t>(floats, 4) * sizeof(float));
        if (e != hipSuccess) return fail(h, MSR_ERR_DEVICE, "hipMemset for %s failed", key.c_str());
    }
    h->dev[key] = p;
    h->dev_bytes[key] = floats * sizeof(float);
    h->dev_zeroed[key] = zero;
    h->total_bytes += floats * sizeof(float);
    *out = p;
    return MSR_OK;
}

int upload(msr_handle* h, const std::string& key, const float* host, size_t floats) {
    float* d = nullptr;
    int rc = dev_alloc(h, key, floats, false, &d);
    if (rc) return rc;
    HIPCHK(h, hipMemcpy(d, host, floats * sizeof(float), hipMemcpyHostToDevice));
    return MSR_OK;
}

float* D(msr_handle* h, const std::string& key) {
    auto it = h->dev.find(key);
    return it == h->dev.end() ? nullptr : it->second;
}

}  // namespace msr

static void add_spec(msr_handle* h, const std::string& name, std::vector<int64_t> shape, WeightKind kind, int i = 0, int j = 0,
                     bool flag = false) {
    h->spec_index[name] = (int)h->specs.size();
    h->specs.push_back({name, std::move(shape), kind, i, j, flag, false});
}

// The weights a handle expects, in load order: public names (msr_weight_name, the Python loaders), shapes, and what
// msr_load_weight does with each (WeightKind and its indices).
static void build_specs(msr_handle* h) {
    char n[128];
    if (h->variant == MSR_PIX2PIX) {
        int cin = 2;
        for (int i = 1; i <= 8; ++i) {
            const int c = kP2PDown[i - 1];
            snprintf(n, sizeof n, "p2p.down%d.kernel", i); add_spec(h, n, {4, 4, cin, c}, i == 1 ? W_P2P_DIRECT : W_P2P_DOWN);
            if (i > 1)
                for (const char* q : {"gamma", "beta", "moving_mean", "moving_variance"}) {
                    snprintf(n, sizeof n, "p2p.down%d.bn.%s", i, q); add_spec(h, n, {c}, W_P2P_SMALL);
                }
            cin = c;
        }
        for (int i = 1; i <= 7; ++i) {
            const int c = kP2PUp[i - 1];
            snprintf(n, sizeof n, "p2p.up%d.kernel", i); add_spec(h, n, {4, 4, c, cin}, W_P2P_UP);
            for (const char* q : {"gamma", "beta", "moving_mean", "moving_variance"}) {
                snprintf(n, sizeof n, "p2p.up%d.bn.%s", i, q); add_spec(h, n, {c}, W_P2P_SMALL);
            }
            cin = c + kP2PDown[6 - (i - 1)];
        }
        add_spec(h, "p2p.last.kernel", {4, 4, 1, cin}, W_P2P_LAST);
        add_spec(h, "p2p.last.bias", {1}, W_P2P_SMALL);
        return;
    }
    const int S = h->S, L = h->L;
    int cin = 2;
    for (int i = 1; i <= 5; ++i) {
        const int c = kEncChannels[i - 1];
        snprintf(n, sizeof n, "enc.ds%d.kernel", i); add_spec(h, n, {3, 3, cin, c}, i == 1 ? W_REF_LAYOUT : W_ENC_CONV_KERNEL, i);
        if (i > 1) {
            snprintf(n, sizeof n, "enc.ds%d.in.gamma", i); add_spec(h, n, {c}, W_REF_LAYOUT);
            snprintf(n, sizeof n, "enc.ds%d.in.beta", i); add_spec(h, n, {c}, W_REF_LAYOUT);
        }
        cin = c;
    }
    const int64_t flat = (int64_t)(S / 32) * (S / 32) * 512;
    for (const bool variance : {false, true}) {
        const char* q = variance ? "variance" : "mean";
        snprintf(n, sizeof n, "enc.%s.kernel", q); add_spec(h, n, {flat, L}, W_ENC_HEAD_KERNEL, 0, 0, variance);
        snprintf(n, sizeof n, "enc.%s.bias", q); add_spec(h, n, {L}, W_ENC_HEAD_BIAS, 0, 0, variance);
    }
    const int sw = S / 64;
    add_spec(h, "gen.dense.kernel", {L, (int64_t)sw * sw * 1024}, W_REF_LAYOUT);
    add_spec(h, "gen.dense.bias", {(int64_t)sw * sw * 1024}, W_REF_LAYOUT);
    cin = 1024;
    for (int i = 1; i <= 6; ++i) {
        const int f = kGenFilters[i - 1];
        const bool learned = f != cin;
        for (int j = 1; j <= (learned ? 3 : 2); ++j) {
            const int c = j == 2 ? f : cin;
            snprintf(n, sizeof n, "gen.rb%d.spade_%d.conv.kernel", i, j); add_spec(h, n, {3, 3, 2, 128}, W_SPADE_EMBED_KERNEL, i, j);
            snprintf(n, sizeof n, "gen.rb%d.spade_%d.conv.bias", i, j); add_spec(h, n, {128}, W_SPADE_EMBED_BIAS, i, j);
            snprintf(n, sizeof n, "gen.rb%d.spade_%d.conv_gamma.kernel", i, j); add_spec(h, n, {3, 3, 128, c}, W_GB_KERNEL, i, j, false);
            snprintf(n, sizeof n, "gen.rb%d.spade_%d.conv_gamma.bias", i, j); add_spec(h, n, {c}, W_GB_BIAS, i, j, false);
            snprintf(n, sizeof n, "gen.rb%d.spade_%d.conv_beta.kernel", i, j); add_spec(h, n, {3, 3, 128, c}, W_GB_KERNEL, i, j, true);
            snprintf(n, sizeof n, "gen.rb%d.spade_%d.conv_beta.bias", i, j); add_spec(h, n, {c}, W_GB_BIAS, i, j, true);
        }
        for (int j = 1; j <= (learned ? 3 : 2); ++j) {
            const int ci = j == 2 ? f : cin;
            snprintf(n, sizeof n, "gen.rb%d.conv_%d.kernel", i, j); add_spec(h, n, {3, 3, ci, f}, W_GEN_CONV_KERNEL, i, j);
            snprintf(n, sizeof n, "gen.rb%d.conv_%d.bias", i, j); add_spec(h, n, {f}, W_REF_LAYOUT);
        }
        cin = f;
    }
    add_spec(h, "gen.head.kernel", {4, 4, 128, 1}, W_HEAD_KERNEL);
    add_spec(h, "gen.head.bias", {1}, W_HEAD_BIAS);
}

// Uploads the [taps][N][Cin] weights `host` of a conv as the image its form reads, under `key` (+ key.wexp: the per-channel
// scales of the fp8 / f16c images).  The images are built on the host by weight_images.hip; this is the one place that puts
// them on the device.
static int upload_conv_weight(msr_handle* h, const std::string& key, const float* host, int taps, int N, int Cin, WeightImage img) {
    h->dev_img[key] = img;
    std::vector<float> image;
    std::vector<int> wexp;
    switch (img) {
        case IMG_F32: return upload(h, key, host, (size_t)taps * N * Cin);
        case IMG_BF16:
        case IMG_BF16_FRAG:
        case IMG_F16:
            if (N % 32 || Cin % 32)
                return fail(h, MSR_ERR_INVALID, "%s: bf16x3 needs Cin and Cout multiples of 32", key.c_str());
            image = build_split_image(host, taps, N, Cin, img);
            break;
        case IMG_FP8: image = build_fp8_image(host, taps, N, Cin, wexp); break;
        case IMG_F16C:
            if (Cin % 32) return fail(h, MSR_ERR_INVALID, "%s: f16c needs Cin %% 32 == 0", key.c_str());
            image = build_f16c_image(host, taps, N, Cin, wexp);
            break;
        case IMG_F16C6:
            if (Cin % 32) return fail(h, MSR_ERR_INVALID, "%s: f16c6 needs Cin %% 32 == 0", key.c_str());
            image = build_f16c6_image(host, taps, N, Cin);
            break;
        case IMG_GBR:
            if (taps != 9 || Cin != 128)
                return fail(h, MSR_ERR_INVALID, "%s: conv_gb_resident takes 3x3 x 128 inputs", key.c_str());
            image = gbr_weight_stream(host, N);
            break;
    }
    int rc = upload(h, key, image.data(), image.size());
    if (rc || wexp.empty()) return rc;
    return upload(h, key + ".wexp", reinterpret_cast<const float*>(wexp.data()), wexp.size());
}

// The half of msr_create that touches no device: validates cfg and fills the handle's configuration (all that fill_forms reads).
int msr::configure(msr_handle* h, const msr_config* cfg) {
    const int S = cfg->image_size, B = cfg->batch_size;
    if (cfg->variant < MSR_GAUGAN || cfg->variant > MSR_PIX2PIX)
        return fail(nullptr, MSR_ERR_INVALID, "unknown variant %d", cfg->variant);
    if (cfg->variant == MSR_PIX2PIX) {
        if (S != 256) return fail(nullptr, MSR_ERR_INVALID, "pix2pix input is fixed to 256x256 (pix2pix.py:7), got %d", S);
    } else {
        if (S < 64 || (S & (S - 1)))
            return fail(nullptr, MSR_ERR_INVALID, "image_size must be a power of two >= 64, got %d", S);
        if (cfg->latent_dim <= 0 || cfg->latent_dim % 4)
            return fail(nullptr, MSR_ERR_INVALID, "latent_dim must be a positive multiple of 4, got %d", cfg->latent_dim);
    }
    if (B < 1 || B > 16) return fail(nullptr, MSR_ERR_INVALID, "batch_size must be in [1,16], got %d", B);
    h->cfg = *cfg;
    h->S = S; h->B = B; h->L = cfg->latent_dim; h->variant = cfg->variant;
    h->prec = (cfg->flags & MSR_FLAG_BF16X3) ? PREC_BF16X3 : PREC_F32;
    h->gb_f16x2 = h->prec == PREC_BF16X3 && (cfg->flags & MSR_FLAG_GB_F16X2);
    if ((cfg->flags & MSR_FLAG_GB_F16X2) && !(cfg->flags & MSR_FLAG_BF16X3))
        return fail(nullptr, MSR_ERR_INVALID, "MSR_FLAG_GB_F16X2 needs MSR_FLAG_BF16X3");
    if ((cfg->flags & MSR_FLAG_FP8) && (!(cfg->flags & MSR_FLAG_BF16X3) || (cfg->flags & MSR_FLAG_GB_F16X2)))
        return fail(nullptr, MSR_ERR_INVALID, "MSR_FLAG_FP8 goes with MSR_FLAG_BF16X3 alone (the layers it does not cover run bf16x3)");
    h->fp8 = (cfg->flags & MSR_FLAG_FP8) && cfg->variant != MSR_PIX2PIX;
    if ((cfg->flags & MSR_FLAG_F16C) && (!(cfg->flags & MSR_FLAG_BF16X3) || (cfg->flags & (MSR_FLAG_GB_F16X2 | MSR_FLAG_FP8))))
        return fail(nullptr, MSR_ERR_INVALID, "MSR_FLAG_F16C goes with MSR_FLAG_BF16X3 alone (the layers it does not cover run bf16x3)");
    h->f16c = (cfg->flags & MSR_FLAG_F16C) && cfg->variant != MSR_PIX2PIX;
    if ((cfg->flags & MSR_FLAG_F16_MAIN) && !(cfg->flags & MSR_FLAG_F16C))
        return fail(nullptr, MSR_ERR_INVALID, "MSR_FLAG_F16_MAIN modifies MSR_FLAG_F16C");
    h->f16m = h->f16c && (cfg->flags & MSR_FLAG_F16_MAIN);
    if ((cfg->flags & MSR_FLAG_CROSS_FP6) && (!(cfg->flags & MSR_FLAG_F16C) || (cfg->flags & MSR_FLAG_F16_MAIN)))
        return fail(nullptr, MSR_ERR_INVALID, "MSR_FLAG_CROSS_FP6 modifies MSR_FLAG_F16C and does not go with MSR_FLAG_F16_MAIN (which computes no cross terms)");
    h->cross6 = h->f16c && (cfg->flags & MSR_FLAG_CROSS_FP6);
    if (cfg->flags & MSR_FLAG_FUSED_HEAD) {
        if (!(cfg->flags & MSR_FLAG_F16C))
            return fail(nullptr, MSR_ERR_INVALID, "MSR_FLAG_FUSED_HEAD needs MSR_FLAG_F16C (the head epilogue exists in the f16c stream kernel)");
        if (cfg->flags & (MSR_FLAG_F16_MAIN | MSR_FLAG_CROSS_FP6))
            return fail(nullptr, MSR_ERR_INVALID, "MSR_FLAG_FUSED_HEAD does not go with MSR_FLAG_F16_MAIN or MSR_FLAG_CROSS_FP6 (they run "
                        "other instantiations of the stream kernel, which have no head epilogue)");
        if (cfg->variant == MSR_PIX2PIX)
            return fail(nullptr, MSR_ERR_INVALID, "MSR_FLAG_FUSED_HEAD serves the SPADE head only, not variant pix2pix");
        h->fused_head = true;
    }
    if (cfg->variant == MSR_PIX2PIX) { h->prec = PREC_F32; h->gb_f16x2 = false; }   // the parity config runs on the fp32 MFMA
    return MSR_OK;
}

// ================================================================================================
extern "C" {

int msr_abi_version(void) { return MSR_ABI_VERSION; }

uint32_t msr_crc32c(const void* host_data, uint64_t n, uint32_t crc) {
    static uint32_t table[8][256];
    static bool ready = false;
    if (!ready) {   // slicing-by-8 tables, reflected polynomial 0x82F63B78
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            table[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int t = 1; t < 8; ++t) table[t][i] = (table[t - 1][i] >> 8) ^ table[0][table[t - 1][i] & 0xFF];
        ready = true;
    }
    const uint8_t* p = static_cast<const uint8_t*>(host_data);
    uint32_t c = crc ^ 0xFFFFFFFFu;
    while (n >= 8) {
        uint32_t lo, hi;
        std::memcpy(&lo, p, 4);
        std::memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = table[7][lo & 0xFF] ^ table[6][(lo >> 8) & 0xFF] ^ table[5][(lo >> 16) & 0xFF] ^ table[4][lo >> 24] ^
            table[3][hi & 0xFF] ^ table[2][(hi >> 8) & 0xFF] ^ table[1][(hi >> 16) & 0xFF] ^ table[0][hi >> 24];
        p += 8;
        n -= 8;
    }
    while (n--) c = table[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

const char* msr_last_error(const msr_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int msr_create(const msr_config* cfg, msr_handle** out) {
    if (!cfg || !out) return fail(nullptr, MSR_ERR_INVALID, "msr_create: null argument");
    *out = nullptr;
    auto h = std::make_unique<msr_handle>();
    if (int rc = configure(h.get(), cfg)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, MSR_ERR_DEVICE, "no HIP device visible: libmoonsr_hip has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, MSR_ERR_DEVICE, "device %d out of range (%d visible)", cfg->device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
        return fail(nullptr, MSR_ERR_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MSR_ERR_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only",
                    cfg->device, prop.gcnArchName);
    if (hipSetDevice(cfg->device) != hipSuccess) return fail(nullptr, MSR_ERR_DEVICE, "hipSetDevice failed");
#ifdef MSR_DIAG_BUILD   // stamp / what-if object (kernels.h): never the product
    if (env_int("MSR_ALLOW_DIAG_BUILD", 0) != 1)
        return fail(nullptr, MSR_ERR_STATE, "this libmoonsr_hip.so is a diagnostic build (-DMSR_DIAG_BUILD: in-kernel stamps "
                    "or what-if switches that change results); set MSR_ALLOW_DIAG_BUILD=1 to use it for measurements");
#endif
    if (conv_igemm_init() != hipSuccess || conv_gbr_init() != hipSuccess)
        return fail(nullptr, MSR_ERR_DEVICE, "could not set the dynamic-LDS attribute of the conv kernels");
    build_specs(h.get());
    fill_forms(h.get());
    *out = h.release();
    return MSR_OK;
}

int msr_destroy(msr_handle* h) {
    if (!h) return MSR_OK;
    hipSetDevice(h->cfg.device);
    hipDeviceSynchronize();
    for (auto& g : h->graphs) {
        if (g.exec) hipGraphExecDestroy(g.exec);
        if (g.graph) hipGraphDestroy(g.graph);
    }
    for (auto& kv : h->dev) hipFree(kv.second);
    if (h->mom_partial) hipFree(h->mom_partial);
    if (h->dense_partial) hipFree(h->dense_partial);
    if (h->conv_partial) hipFree(h->conv_partial);
    if (h->stat_ws) hipFree(h->stat_ws);
    if (h->window) hipFree(h->window);
    if (h->stitch_grid) hipFree(h->stitch_grid);
    for (auto e : h->ev_pool) hipEventDestroy(e);
    for (auto& op : h->ops)
        if (op.done) hipEventDestroy(op.done);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->aux) hipStreamDestroy(h->aux);
    if (h->range_table_dev) hipFree(h->range_table_dev);
    if (h->range_rec_dev) hipFree(h->range_rec_dev);
    if (h->range_rec_host) hipHostFree(h->range_rec_host);
    if (h->range_done) hipEventDestroy(h->range_done);
    delete h;
    return MSR_OK;
}

int msr_weight_count(const msr_handle* h, int32_t* expected, int32_t* loaded) {
    if (!h) return MSR_ERR_INVALID;
    int l = 0;
    for (auto& s : h->specs) l += s.loaded;
    if (expected) *expected = (int32_t)h->specs.size();
    if (loaded) *loaded = l;
    return MSR_OK;
}

const char* msr_weight_name(const msr_handle* h, int32_t i, int64_t* shape4, int32_t* rank) {
    if (!h || i < 0 || i >= (int)h->specs.size()) return nullptr;
    const auto& s = h->specs[i];
    if (rank) *rank = (int32_t)s.shape.size();
    if (shape4)
        for (size_t k = 0; k < s.shape.size() && k < 4; ++k) shape4[k] = s.shape[k];
    return s.name.c_str();
}

int msr_load_weight(msr_handle* h, const char* name_c, const float* host, const int64_t* shape, int32_t rank) {
    if (!h) return MSR_ERR_INVALID;
    if (!name_c || !host || !shape) return fail(h, MSR_ERR_INVALID, "msr_load_weight: null argument");
    const std::string name = name_c;
    auto it = h->spec_index.find(name);
    if (it == h->spec_index.end()) return fail(h, MSR_ERR_INVALID, "unexpected weight name '%s'", name_c);
    WeightSpec& sp = h->specs[it->second];
    if (rank != (int)sp.shape.size()) return fail(h, MSR_ERR_INVALID, "%s: rank %d, expected %zu", name_c, rank, sp.shape.size());
    size_t count = 1;
    for (int k = 0; k < rank; ++k) {
        if (shape[k] != sp.shape[k])
            return fail(h, MSR_ERR_INVALID, "%s: dim %d is %lld, expected %lld", name_c, k, (long long)shape[k],
                        (long long)sp.shape[k]);
        count *= (size_t)shape[k];
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->planned = false;
    int rc = MSR_OK;
    const auto& s = sp.shape;
    // Conv2DTranspose(k=4, s=2, 'same') is four stride-1 2x2 convolutions, one per output parity (py, px):
    // out[2y+py][2x+px] = sum_{t,u} in[y-1+py+t][x-1+px+u] * W[kmap(py,t)][kmap(px,u)], kmap(0,.) = {3,1},
    // kmap(1,.) = {2,0}  (from kh = o + 1 - 2i, the transpose of the 'same' stride-2 forward conv).
    static const int kmap[2][2] = {{3, 1}, {2, 0}};
    char base[64];   // gen.rb<i>.spade_<j>: the combined gamma|beta tensors live under it
    snprintf(base, sizeof base, "gen.rb%d.spade_%d", sp.i, sp.j);
    switch (sp.kind) {
        case W_P2P_DIRECT:
            rc = upload(h, name, host, count);                       // conv_direct reads HWIO
            break;
        case W_P2P_LAST: {
            // [4,4,1,C] -> the head kernel's effective taps weff[py][px][dy][dx][C], offset dy-1 = py+t-1
            const std::vector<float> weff = head_weff_transpose(host, (int)s[3]);
            rc = upload(h, "p2p.last.weff", weff.data(), weff.size());
            break;
        }
        case W_P2P_UP: {
            // [kh,kw,Cout,Cin] is already K-contiguous per output channel: four parity images [2x2 taps][Cout][Cin]
            const size_t co = (size_t)s[2], ci = (size_t)s[3];
            std::vector<float> t4(count);
            for (int py = 0; py < 2; ++py)
                for (int px = 0; px < 2; ++px)
                    for (int t = 0; t < 2; ++t)
                        for (int u = 0; u < 2; ++u) {
                            const float* src = host + ((size_t)kmap[py][t] * 4 + kmap[px][u]) * co * ci;
                            std::copy(src, src + co * ci, t4.data() + ((size_t)(py * 2 + px) * 4 + t * 2 + u) * co * ci);
                        }
            rc = upload(h, name, t4.data(), count);
            h->dev_img[name] = IMG_F32;
            break;
        }
        case W_P2P_DOWN: {
            // down2..8: HWIO -> [tap][Cout][Cin]
            std::vector<float> t(count);
            hwio_to_tap_oc_ic(host, t.data(), 16, (int)s[2], (int)s[3], (int)s[3], nullptr);
            rc = upload(h, name, t.data(), count);
            h->dev_img[name] = IMG_F32;
            break;
        }
        case W_P2P_SMALL:
        case W_HEAD_BIAS:
            h->host_small[name].assign(host, host + count);   // BN statistics / bias: folded at plan time
            break;
        case W_SPADE_EMBED_KERNEL:
        case W_SPADE_EMBED_BIAS:
            h->host_small[name].assign(host, host + count);   // msr_range_embed_bounds reads the fp32 embedding weights
            rc = upload(h, name, host, count);
            if (!rc && sp.kind == W_SPADE_EMBED_KERNEL) {
                // conv_gb_resident multiplies the mask embedding on the fp16 MFMA: its A operands (three fp16 terms per product)
                std::vector<float> e16(4096);
                conv_gbr_embed_image(host, e16.data());
                rc = upload(h, name + ".e16", e16.data(), e16.size());
            }
            break;
        case W_REF_LAYOUT:
            rc = upload(h, name, host, count);   // used in the reference layout
            break;
        case W_ENC_HEAD_KERNEL: {
            // concatenate the two heads into one [K, 2L] matrix so the flatten is streamed once
            float* d = nullptr;
            rc = dev_alloc(h, "enc.heads.kernel", (size_t)s[0] * 2 * h->L, false, &d);
            if (!rc) {
                const size_t coff = sp.flag ? (size_t)h->L : 0;
                HIPCHK(h, hipMemcpy2D(d + coff, (size_t)2 * h->L * sizeof(float), host, (size_t)h->L * sizeof(float),
                                      (size_t)h->L * sizeof(float), (size_t)s[0], hipMemcpyHostToDevice));
            }
            break;
        }
        case W_ENC_HEAD_BIAS: {
            float* d = nullptr;
            rc = dev_alloc(h, "enc.heads.bias", (size_t)2 * h->L, false, &d);
            if (!rc) HIPCHK(h, hipMemcpy(d + (sp.flag ? h->L : 0), host, h->L * sizeof(float), hipMemcpyHostToDevice));
            break;
        }
        case W_HEAD_KERNEL: {
            // effective per-parity taps of Conv2D(1,4,'same') applied to a nearest-2x up-sampled tensor: for head_kernel, or,
            // where the plan fuses the head, as fp16 hi | lo MFMA fragments for conv_sw.hip's sw_epilogue_head
            if (head_fused_form(h)) {
                const std::vector<float> wfrag = build_head_wfrag(host);
                rc = upload(h, "gen.head.wfrag", wfrag.data(), wfrag.size());
                break;
            }
            const std::vector<float> weff = head_weff_upconv(host, (int)s[2]);
            rc = upload(h, "gen.head.weff", weff.data(), weff.size());
            break;
        }
        case W_GB_KERNEL: {
            // gamma and beta convs share their input: ONE GEMM with N = 2C whose columns interleave
            // (32 gamma channels | 32 beta channels) so a wave holds both for the same pixel and channel.
            const int cin = (int)s[2], C = (int)s[3];
            std::vector<int> rowmap(C);
            for (int c = 0; c < C; ++c) rowmap[c] = (c / 32) * 64 + (sp.flag ? 32 : 0) + (c % 32);
            // stage through a host image of the combined tensor; the other half is filled by the sibling call
            const std::string key = std::string(base) + ".gb.kernel";
            std::vector<float>& img = h->host_small[key];
            img.resize((size_t)9 * 2 * C * cin);
            hwio_to_tap_oc_ic(host, img.data(), 9, cin, C, 2 * C, rowmap.data());
            rc = upload_conv_weight(h, key, img.data(), 9, 2 * C, cin, h->spade_forms[sp.i][sp.j].gb.img);
            break;
        }
        case W_GB_BIAS: {
            const int C = (int)s[0];
            const std::string key = std::string(base) + ".gb.bias";
            std::vector<float>& img = h->host_small[key];
            img.resize((size_t)2 * C);
            for (int c = 0; c < C; ++c) img[(c / 32) * 64 + (sp.flag ? 32 : 0) + (c % 32)] = host[c];
            rc = upload(h, key, img.data(), img.size());
            break;
        }
        case W_ENC_CONV_KERNEL:
        case W_GEN_CONV_KERNEL: {
            // encoder ds2..5 and ResidualBlock conv_1/2/3 (conv_j is fed by spade_j): HWIO -> [tap][Cout][Cin]
            const int taps = (int)(s[0] * s[1]), cin = (int)s[2], cout = (int)s[3];
            std::vector<float> t(count);
            hwio_to_tap_oc_ic(host, t.data(), taps, cin, cout, cout, nullptr);
            const ConvForm& form = sp.kind == W_GEN_CONV_KERNEL ? h->spade_forms[sp.i][sp.j].cv : h->enc_forms[sp.i];
            rc = upload_conv_weight(h, name, t.data(), taps, cout, cin, form.img);
            break;
        }
    }
    if (rc) return rc;
    sp.loaded = true;
    return MSR_OK;
}

}  // extern "C"

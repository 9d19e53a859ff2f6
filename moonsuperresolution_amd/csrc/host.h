// host.h — what the host units of libmoonsr_hip.so share: the handle, the planned op, the weight specs, the conv forms, the
// error plumbing, the device-buffer table and the few functions one unit calls in another.  Host logic only; the launch
// interface of the kernels is kernels.h.  Units: api.hip (handle, weight loader), weight_images.hip, forms.hip, plan.hip,
// forward.hip, op_entries.hip, debug_entries.hip, tiler_entries.hip.
#pragma once
#include "../../include/moonsr.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace msr {

// What msr_load_weight does with a weight: one value per branch of the loader.  build_specs sets it where it builds the name.
enum WeightKind {
    W_P2P_DIRECT,          // p2p.down1.kernel: conv_direct reads HWIO
    W_P2P_DOWN,            // p2p.down2..8.kernel: HWIO -> [tap][Cout][Cin]
    W_P2P_UP,              // p2p.up1..7.kernel: Conv2DTranspose as four parity images
    W_P2P_LAST,            // p2p.last.kernel -> p2p.last.weff
    W_P2P_SMALL,           // BN statistics / bias: host copy, folded at plan time
    W_REF_LAYOUT,          // uploaded in the reference layout
    W_SPADE_EMBED_KERNEL,  // gen.rb<i>.spade_<j>.conv.kernel: reference layout + host copy + the .e16 image
    W_SPADE_EMBED_BIAS,    // gen.rb<i>.spade_<j>.conv.bias: reference layout + host copy
    W_ENC_HEAD_KERNEL,     // enc.mean / enc.variance kernel -> one half of enc.heads.kernel (flag: variance)
    W_ENC_HEAD_BIAS,       // ... bias -> one half of enc.heads.bias (flag: variance)
    W_HEAD_KERNEL,         // gen.head.kernel -> gen.head.weff, or gen.head.wfrag where the plan fuses the head
    W_HEAD_BIAS,           // gen.head.bias: host copy
    W_GB_KERNEL,           // gen.rb<i>.spade_<j>.conv_gamma / conv_beta kernel -> one half of .gb.kernel (flag: beta)
    W_GB_BIAS,             // ... bias -> one half of .gb.bias (flag: beta)
    W_ENC_CONV_KERNEL,     // enc.ds<i>.kernel, i = 2..5: the image of enc_forms[i]
    W_GEN_CONV_KERNEL,     // gen.rb<i>.conv_<j>.kernel: the image of spade_forms[i][j].cv
};

struct WeightSpec {
    std::string name;
    std::vector<int64_t> shape;
    WeightKind kind;
    int i = 0, j = 0;                 // block and layer of the kinds that carry them
    bool flag = false;                // is-beta (W_GB_*) / is-variance (W_ENC_HEAD_*)
    bool loaded = false;
};

enum OpType { OP_CONV, OP_SMALLCIN, OP_MOMENTS, OP_MOMENTS_SLABS, OP_NORMACT, OP_DENSE, OP_LATENT, OP_HEAD, OP_DIRECT, OP_GBR, OP_HEAD_GATHER };

struct Op {
    OpType type;
    double flops = 0, bytes = 0;
    // flags for per-call pointers
    bool src_is_input = false, out_is_output = false, eps_is_input = false;
    bool on_aux = false;              // depends on the call's input only: runs on the handle's auxiliary stream
    hipEvent_t done = nullptr;        // recorded on the auxiliary stream after an on_aux op
    hipEvent_t wait = nullptr;        // the main stream waits for this before launching the op
    int aux_group = -1;               // on_aux ops and their consumers: one event / one wait per group
    ConvParams conv{}; int epi = 0, tile = 0, kernel = KERNEL_GENERIC;   // the form's ConvKernel and tile geometry
    int stat_slabs = 0;               // > 0: the conv's epilogue also writes partial output moments (fused)
    SmallCinParams sc{};
    GbrParams gbr{}; int gbr_ranges = 0;   // OP_GBR: mask embedding + gamma|beta conv + SPADE epilogue in one launch (conv_gbr.hip)
                                           // in the SpadeForm's `ranges` work items per pixel tile
    struct { const float* x; int G, P, C; float eps; float* mean; float* stdv; } mom{};
    NormActParams na{};
    struct { const float* x; const float* W; const float* bias; float* y; int B, K, N; } dense{};
    struct { const float* mv; float* z; int B, L, sampler; } lat{};
    struct { const float* x; const float* weff; float bias; int B, r, C; float slope; int tanh_out; int x_py, x_pb; } head{};
    DirectConvParams dc{};
    struct { const float* partial; float bias; int B, r; } hg{};   // OP_HEAD_GATHER: the fused head's second launch
};

struct ProfRec { int fam; hipEvent_t a, b; double flops, bytes; int launches; };

// Weight image of a conv: what msr_load_weight builds from the [taps][N][Cin] kernel layout (upload_conv_weight)
enum WeightImage {
    IMG_F32,         // fp32 as is
    IMG_BF16,        // split-bf16 words: every 32 consecutive k become [32 hi | 32 lo]
    IMG_BF16_FRAG,   // split-bf16 in MFMA-fragment order (conv_igemm_bf16x3: B fragments straight to VGPRs)
    IMG_F16,         // split-fp16 words (PREC_F16X2)
    IMG_FP8,         // fp8 e4m3 bytes + key.wexp (PREC_FP8)
    IMG_F16C,        // f16c chunk image + key.wexp (PREC_F16C)
    IMG_F16C6,       // f16c6 chunk image, scales inside (PREC_F16C6)
    IMG_GBR,         // the weight stream of conv_gb_resident (gbr_weight_stream)
};

// Form of one conv layer: the kernel that runs it (a ConvKernel, chosen once by conv_kernel_for; launch_conv switches on it) and
// the weight image that kernel reads.  msr_load_weight and the planner both take it from the handle's form table (fill_forms),
// so a layer's weights are always in the layout its launch expects.
struct ConvForm {
    int prec = PREC_F32, tile = TILE_64x64, ksplit = 1, wt_frag = 0, kernel = KERNEL_GENERIC;
    int no_cross = 0;                 // f16 mode: the stream / resident kernels leave the cross terms out
    WeightImage img = IMG_F32;
};

// Form of one SPADE layer of the generator and of the conv it feeds (gen.rbI.spade_J -> gen.rbI.conv_J)
struct SpadeForm {
    int ranges = 0;                   // > 0: conv_gb_resident (embedding + gamma|beta conv + SPADE epilogue in one launch), in
                                      // that many work items per pixel tile (conv_gbr_ranges)
    int h_split = 0, hslots = 128;    // mask embedding (not run under gbr): out_split, float slots per pixel of its output
    ConvForm gb;                      // gamma|beta conv
    int a_split = 0, aslots = 0;      // the format the gamma|beta conv writes for the consumer, float slots per pixel
    ConvForm cv;                      // consumer conv
};

struct Padded {   // zero-bordered NHWC activation [B, r+2, r+2, C]
    float* base = nullptr;
    int r = 0, C = 0;
    int py() const { return (r + 2) * C; }
    int pb() const { return (r + 2) * (r + 2) * C; }
    int interior() const { return py() + C; }
};

}  // namespace msr

struct msr_handle {
    msr_config cfg{};
    int S = 0, B = 0, L = 0, variant = 0;
    int prec = 0;                                // PREC_F32 or PREC_BF16X3 (cfg.flags & MSR_FLAG_BF16X3)
    bool gb_f16x2 = false;                       // MSR_FLAG_GB_F16X2: 2-term fp16 products in the gamma|beta convs
    bool fp8 = false;                            // MSR_FLAG_FP8: declared non-parity mode (fp8 weights x bf8 activations)
    bool f16c = false;                           // MSR_FLAG_F16C: fp16 main term + fp8 cross terms in the chip-filling convs
    bool f16m = false;                           // MSR_FLAG_F16_MAIN: F16C without the cross terms in the stream / resident kernels
    bool cross6 = false;                         // MSR_FLAG_CROSS_FP6: fp6 cross terms in the stream-kernel consumers of F16C
    bool fused_head = false;                     // MSR_FLAG_FUSED_HEAD: the request; head_fused_form() says whether the plan takes it
    msr::ConvForm enc_forms[6];                  // [i]: enc.ds<i> (i = 2..5)
    msr::SpadeForm spade_forms[7][4];            // [i][j]: gen.rb<i>.spade_<j> and gen.rb<i>.conv_<j> (i = 1..6, j = 1..3)
    std::string err;
    std::vector<msr::WeightSpec> specs;
    std::map<std::string, int> spec_index;
    std::map<std::string, float*> dev;          // device tensors: weights (re-laid-out) and workspace
    std::map<std::string, size_t> dev_bytes;
    std::map<std::string, bool> dev_zeroed;      // dev_alloc zero-filled the buffer (msr_debug_workspace_list)
    struct PaddedInfo { int r, C, written; };    // alloc_padded: [B, r + 2, r + 2, C], the producer writes `written` slots per pixel
    std::map<std::string, PaddedInfo> dev_padded;
    std::map<std::string, int> dev_img;          // WeightImage of every conv weight uploaded by upload_conv_weight
    std::map<std::string, std::vector<float>> host_small;   // small host copies needed at plan time (BN, head)
    size_t total_bytes = 0;
    bool planned = false;
    std::vector<msr::Op> ops;
    double fwd_flops = 0;
    double* mom_partial = nullptr;
    float* dense_partial = nullptr;
    size_t mom_partial_bytes = 0, dense_partial_bytes = 0;   // as counted in total_bytes
    float* conv_partial = nullptr;     // split-K workspace [ksplit][M][N]
    size_t conv_partial_floats = 0;
    float* stat_ws = nullptr;          // fused-moments slabs [P][3][N] of the conv that ran last
    size_t stat_ws_floats = 0;
    float* z = nullptr;
    // tiler
    double* window = nullptr;     // [S-2p, S-2p] float64
    int* stitch_grid = nullptr;
    int stitch_grid_cap = 0;
    // auxiliary stream: the SPADE mask embeddings depend only on the call's input, so they are launched on a
    // second stream and overlap the encoder and the low-resolution (latency-bound) layers
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr;
    // HIP graphs of the launch plan, one per (input, noise, output) pointer triple (msr_graph_enable)
    struct GraphEntry { const float* in; const float* eps; float* out; hipGraph_t graph; hipGraphExec_t exec; uint64_t last_use; };
    struct Triple { const float* in; const float* eps; float* out; };
    int graph_on = 0;
    std::vector<GraphEntry> graphs;              // at most 8, least recently used evicted
    std::vector<Triple> seen_once;               // triples run eagerly once: a triple is captured on its SECOND sighting
    uint64_t graph_clock = 0;
    int gate_op = -1;                            // index of the first op of the matrix-bound part (msr_forward_gated)
    // profiling
    int prof_on = 0;                               // 0 off, 1 every launch, 2 runs of conv launches only
    std::vector<msr::ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    // activation-range scan (msr_range_scan): the narrow activation tensors of the plan, in plan order.  Nothing here is
    // allocated on the device before the first scan.
    struct RangeEntry { std::string tensor; int producer; msr::RangeScanItem item; };
    struct EmbedEntry { std::string kernel; int producer; };
    std::vector<RangeEntry> range_plan;
    std::vector<EmbedEntry> range_embeds;        // the gbr ops, whose embedding exists only in LDS (msr_range_embed_bounds)
    msr::RangeScanItem* range_table_dev = nullptr;
    msr::RangeScanRecord* range_rec_dev = nullptr;
    msr::RangeScanRecord* range_rec_host = nullptr;   // pinned
    size_t range_cap = 0;                        // entries the three buffers hold
    bool range_table_stale = true;
    hipEvent_t range_done = nullptr;
    bool range_enqueued = false;
    bool forward_seen = false;
};

namespace msr {

// ---- api.hip: errors and the handle's device buffers ----
int fail(msr_handle* h, int code, const char* fmt, ...);   // h == nullptr: the error of msr_create
int configure(msr_handle* h, const msr_config* cfg);       // msr_create's device-free half: validates cfg, fills h's configuration

#define HIPCHK(h, call)                                                                                     \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(h, MSR_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                          \
    } while (0)

inline constexpr int kGenFilters[6] = {1024, 1024, 1024, 512, 256, 128};
inline constexpr int kEncChannels[5] = {64, 128, 256, 512, 512};
inline constexpr int kP2PDown[8] = {64, 128, 256, 512, 512, 512, 512, 512};
inline constexpr int kP2PUp[7] = {512, 512, 512, 512, 256, 128, 64};

int dev_alloc(msr_handle* h, const std::string& key, size_t floats, bool zero, float** out);
int upload(msr_handle* h, const std::string& key, const float* host, size_t floats);
float* D(msr_handle* h, const std::string& key);
// Key of the device buffer that contains ptr (a pointer into a buffer, such as the interior of a padded input, names the
// buffer); nullptr when ptr is null or in none.
const char* name_of(const msr_handle* h, const void* ptr);

// ---- weight_images.hip: host arrays -> host arrays, no handle, no HIP call ----
void hwio_to_tap_oc_ic(const float* src, float* dst, int taps, int cin, int cout, int dst_rows, const int* rowmap);
std::vector<float> build_split_image(const float* host, int taps, int N, int Cin, WeightImage img);
std::vector<float> build_f16c_image(const float* host, int taps, int N, int Cin, std::vector<int>& wexp);
std::vector<float> build_f16c6_image(const float* host, int taps, int N, int Cin);
std::vector<float> build_fp8_image(const float* host, int taps, int N, int Cin, std::vector<int>& wexp);
std::vector<float> gbr_weight_stream(const float* w_tap_n_k, int N);
std::vector<float> head_weff_upconv(const float* k44c, int C);
std::vector<float> head_weff_transpose(const float* k44c, int C);
std::vector<float> build_head_wfrag(const float* k44c);       // gen.head.wfrag: the stream kernel's head epilogue (C = 128)
int fp8_pad(int cin);

// ---- forms.hip ----
ConvForm make_form(int prec, int tile, int ksplit, int cin, int epi, int out_split = OUT_F32, int wt_frag = 0, int no_cross = 0);
ConvForm conv_form(int B, int rout, int N, int stride, int epi, int prec, int cin, int taps = 9);
void fill_forms(msr_handle* h);
// MSR_FLAG_FUSED_HEAD is set and gen.rb6.conv_2 runs the whole-tile stream-kernel form the head epilogue exists for
bool head_fused_form(const msr_handle* h);

// ---- plan.hip ----
Op conv_op(const Padded& in, int cin, const float* wt, const float* bias, int B, int rout, int N, int stride, int epi,
           const ConvForm& f);
int ensure_plan(msr_handle* h);
int ensure_conv_partial(msr_handle* h, size_t floats);
void drop_graphs(msr_handle* h);

// Output / aux views of the parameter structs that share the field names (ConvParams, SmallCinParams, GbrParams,
// NormActParams): a dense [B, H, W, C] tensor, or the interior of a zero-bordered [B, H + 2, W + 2, C] one.
template <class P> void set_out_dense(P& p, float* out, int H, int W, int C) {
    p.out = out; p.out_px = C; p.out_py = W * C; p.out_pb = H * W * C; p.out_off = 0;
}
template <class P> void set_out_padded(P& p, float* base, int H, int W, int C) {
    p.out = base; p.out_px = C; p.out_py = (W + 2) * C; p.out_pb = (H + 2) * (W + 2) * C; p.out_off = p.out_py + C;
}
template <class P> void set_out_padded(P& p, const Padded& o) { set_out_padded(p, o.base, o.r, o.r, o.C); }
template <class P> void set_aux_dense(P& p, const float* x, int rx, int C, int shift) {
    p.aux = x; p.aux_px = C; p.aux_py = rx * C; p.aux_pb = rx * rx * C; p.aux_shift = shift;
}

// ---- debug_entries.hip ----
void range_fill(msr_range_stat* o, const std::string& tensor, int format, int producer, const RangeScanRecord& r);

}  // namespace msr

/*
 * moonsr.h — C ABI of libmoonsr_hip.so, the MI355X (gfx950) implementation of the tiled DEM
 * super-resolution inference path of AntoineRichard/MoonSuperResolution.
 *
 * The reference has NO native interface: its device boundary is the duck-typed Python call
 *     pred = self.model(np.array(batch), training=False)        (process_full_tiles.py:338)
 * on a Keras model built by GauGAN(image_size, batch_size, latent_dim) (process_full_tiles.py:28,
 * spade/models/model.py:340-380) — and its stitcher is NumPy (process_full_tiles.py:363-414).
 * This header is what a binding for that path would bind; INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *  - plain pointers and sizes only; no torch / numpy types.
 *  - every function returns 0 on success or a negative msr_status; msr_last_error() gives the text.
 *  - tensors are NHWC float32; "dev" pointers are HIP device pointers owned by the CALLER.  The
 *    library owns only the weights and the workspace inside the handle.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are asynchronous
 *    on that stream; a handle is not re-entrant.
 *  - there is NO CPU fallback: if no gfx950 device is usable msr_create fails with MSR_ERR_DEVICE.
 *
 * Non-finite inputs
 *  A NaN is data, as it is to the reference (IEEE: relu(NaN) = NaN, 0 * NaN = NaN).  For every kernel entry and for
 *  msr_forward: an output element is NaN exactly where the float64 reference of the same operation is NaN; for an image output
 *  (split-bf16, split-fp16, f16c, f16c6, bf8) that is its MAIN piece (hi, or the bf8 byte), the cross pieces of a NaN element
 *  are unspecified.  Every element that does not depend on a NaN input is bit-identical to the same call with 0.0 in the NaN's
 *  place, cross pieces and block scales of the other channels of a poisoned pixel included (a block scale is the maximum over
 *  the block's non-NaN elements).  Batch statistics (SPADE) hand one sample's NaN to the whole batch, as the reference's do.
 *  +-Inf is outside this contract: the f16c family clamps activations to fp16's range (+-65504) by design, so an infinity
 *  becomes a finite value there (tests/test_gpu_conv_kernel.py::test_f16c_saturation_regimes).
 *  tests/test_gpu_nonfinite.py pins the contract kernel by kernel.
 */
#ifndef MOONSR_H
#define MOONSR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSR_ABI_VERSION 1

typedef enum {
    MSR_OK = 0,
    MSR_ERR_INVALID = -1,   /* bad argument / shape (the reference raises ValueError / assert) */
    MSR_ERR_DEVICE = -2,    /* HIP error or no usable device */
    MSR_ERR_STATE = -3,     /* call out of order (e.g. forward before all weights are loaded) */
    MSR_ERR_NOMEM = -4
} msr_status;

/* Generator families of the reference. */
typedef enum {
    MSR_GAUGAN = 0,        /* GauGAN.call        spade/models/model.py:564-567  z = mean + exp(var/2)*eps */
    MSR_GAUGAN_NO_KL = 1,  /* GauGAN_no_KL.call  spade/models/model.py:265-267  z = mean + var          */
    MSR_CNN = 2,           /* CNNSpade.call      spade/models/model.py:789-791  z = mean + var          */
    MSR_PIX2PIX = 3        /* Pix2Pix().generator  pix2pix.py:88-108 (image_size fixed to 256)            */
} msr_variant;

typedef struct {
    int32_t image_size;  /* S: generator input/output side, power of two >= 64 (GauGAN(image_size, ...)) */
    int32_t batch_size;  /* B: patches per call; baked in like the reference's sampler (sampling.py:13-15) */
    int32_t latent_dim;  /* 256 in every reference script (process_full_tiles.py:28) */
    int32_t variant;     /* msr_variant */
    int32_t device;      /* HIP device ordinal */
    int32_t flags;       /* MSR_FLAG_* */
} msr_config;

/* Conv arithmetic (msr_config.flags).  Inputs, outputs and weights of the C ABI are fp32 in every mode, and so is all
 * other arithmetic (moments, normalisation, epilogues, dense layers, head); only the conv products differ:
 *   0                 exact fp32 on v_mfma_f32_32x32x2_f32 (157 TFLOP/s peak).  NOTE: 0 is the C-ABI default; the Python
 *                     host (moonsuperresolution_amd.Generator) defaults to MSR_FLAG_BF16X3 | MSR_FLAG_F16C, ~4x faster.
 *   MSR_FLAG_BF16X3   3-term split-bf16 products (a_hi*b_hi + a_hi*b_lo + a_lo*b_hi) with fp32 accumulation, on
 *                     v_mfma_f32_16x16x32_bf16 in the LDS-halo kernels (the r >= 16 layers, 91 % of the FLOPs) and on
 *                     v_mfma_f32_32x32x16_bf16 in the small-tile ones: per-product error <= ~3*2^-18.
 *   MSR_FLAG_BF16X3 | MSR_FLAG_GB_F16X2   opt-in: as BF16X3, but the SPADE gamma|beta convs (spade.py:19-20, half of
 *                     the FLOPs) of the layers that run the persistent ping-pong kernel use 2-term fp16 products
 *                     (activation split in two fp16 halves, weight rounded to ONE fp16; v_mfma_f32_16x16x32_f16):
 *                     per-product error <= 2^-12, measured 2-5e-4 relative L-inf end to end (inside north_star's 1e-3,
 *                     with a 2-4x margin instead of 50x; tests/test_gpu_baseline_configs.py states the bound).
 * MSR_PIX2PIX ignores the flags and always computes on the fp32 MFMA. */
#define MSR_FLAG_BF16X3 1
#define MSR_FLAG_GB_F16X2 2
/*   MSR_FLAG_BF16X3 | MSR_FLAG_FP8   declared NON-parity mode (BASELINE.json configs[4], "fp8 MFMA conv"): every 3x3
 *                     stride-1 conv that fills the chip with whole ping-pong tiles (the gamma|beta and ResidualBlock
 *                     convs of the r >= 32 blocks at the BASELINE sizes, ~97 % of the FLOPs) multiplies fp8 e4m3 weights
 *                     (a power-of-two scale per output channel, carried by the instruction's e8m0 scale operand) by bf8
 *                     e5m2 activations on v_mfma_scale_f32_16x16x128_f8f6f4 with fp32 accumulation: 3 and 2 mantissa
 *                     bits per operand.  Its error against the float64 oracle is measured and stated in
 *                     tests/test_gpu_baseline_configs.py; it does NOT meet the 1e-3 bar and is never the default. */
#define MSR_FLAG_FP8 4
/*   MSR_FLAG_BF16X3 | MSR_FLAG_F16C   the same layers as MSR_FLAG_FP8 covers, on "fp16 main term + fp8 cross terms":
 *                     a*b = a_hi*b_hi (v_mfma_f32_16x16x32_f16, exact products) + (a_hi*b_lo + a_lo*b_hi) on the block-scaled fp8
 *                     MFMA (the cross terms are 2^-11 of the product, so 4 bits of them suffice; K = 128 covers both cross
 *                     terms of two taps per instruction at twice the bf16 rate): two MFMA-equivalents per product instead
 *                     of three, per-product error ~2^-15, 3-5e-5 relative L-inf end to end — a parity mode
 *                     (tests/test_gpu_baseline_configs.py). */
#define MSR_FLAG_F16C 8
/*   MSR_FLAG_BF16X3 | MSR_FLAG_F16C | MSR_FLAG_F16_MAIN   declared-tolerance fast mode ("f16", round 3): the F16C data
 *                     path with the cross terms left out of the two kernels that carry ~95 % of the FLOPs (conv_gb_resident,
 *                     conv_igemm_f16c_sw): ONE fp16 product per element on v_mfma_f32_16x16x32_f16, fp32 accumulation,
 *                     per-product error 2^-11.  Tensors, weights and every other layer are exactly F16C's.  It is the usable
 *                     reading of BASELINE.json configs[4] ("fp16 ... conv"): the measured end-to-end error is stated in
 *                     tests/test_gpu_baseline_configs.py::test_f16_mode_declared_tolerance (bound 3e-3 relative L-inf; it is
 *                     NOT inside north_star's 1e-3 and never the default). */
#define MSR_FLAG_F16_MAIN 16
/*   MSR_FLAG_BF16X3 | MSR_FLAG_F16C | MSR_FLAG_CROSS_FP6   opt-in: F16C with the cross terms of the main convs in fp6 e2m3
 *                     with a power-of-two scale per pixel and 32 channels (1.5 MFMA-equivalents per product instead of 2; e2m3
 *                     keeps e4m3's three mantissa bits, so it is the same parity grade).  It covers the consumers that run
 *                     the stream kernel on whole tiles (Cin % 128 == 0); their SPADE layers keep conv_gb_resident, whose
 *                     epilogue writes the fp6 image.  Not valid with MSR_FLAG_F16_MAIN (no cross terms to move); ignored for
 *                     MSR_PIX2PIX.  Not the default: the measured A/B is in DESIGN.md. */
#define MSR_FLAG_CROSS_FP6 32
/*   MSR_FLAG_BF16X3 | MSR_FLAG_F16C | MSR_FLAG_FUSED_HEAD   opt-in: the last residual conv (gen.rb6.conv_2, 128 -> 128 at r = S/2)
 *                     does not write its output; its epilogue applies leaky_relu(0.2) and reduces the 128 channels against the
 *                     head's 25 live per-parity taps, writing 32 partial sums per pixel (ws.gen.head.partial), and a gather
 *                     kernel adds the neighbours' sums and the bias.  The plan takes it when that conv runs the stream kernel
 *                     on whole tiles (B * (S/32)^2 >= 256 tiles); otherwise the separate head runs unchanged (see
 *                     msr_debug_conv_forms: kind=head_gather).  The head's products are three fp16 terms (hi = f16_rn(x),
 *                     lo = f16_rn(x - hi)) accumulated in fp32: within ~1e-6 of the fp32 head, but the fp16 conversion
 *                     SATURATES: an activation beyond 65504 gives a finite, wrong result where the fp32 head has no such limit.
 *                     msr_create returns MSR_ERR_INVALID without MSR_FLAG_F16C, with MSR_FLAG_F16_MAIN or MSR_FLAG_CROSS_FP6,
 *                     and for MSR_PIX2PIX.  Not the default: the measured A/B is in DESIGN.md. */
#define MSR_FLAG_FUSED_HEAD 64

typedef struct msr_handle msr_handle;

/* ---- lifetime -------------------------------------------------------------------------------- */
int msr_abi_version(void);
/* Replaces: GauGAN(image_size, batch_size, latent_dim) + .compile()  (process_full_tiles.py:28-29). */
int msr_create(const msr_config* cfg, msr_handle** out);
int msr_destroy(msr_handle* h);
/* Text of the last error on this handle (h == NULL: last error of a failed msr_create). */
const char* msr_last_error(const msr_handle* h);

/* ---- weights --------------------------------------------------------------------------------- */
/* Replaces: gaugan.load(path+'generator', ..., path+'encoder')  (process_full_tiles.py:30,
 * model.py:607-610).  `host` is a HOST float32 array in the reference's own layout: conv kernels
 * HWIO [kh,kw,Cin,Cout], Conv2DTranspose kernels [kh,kw,Cout,Cin], dense [in,out]; names as listed
 * by moonsuperresolution_amd.weights.weight_shapes().  The library re-lays them out for its kernels. */
int msr_load_weight(msr_handle* h, const char* name, const float* host, const int64_t* shape, int32_t rank);
/* Number of weights the variant expects / has received so far. */
int msr_weight_count(const msr_handle* h, int32_t* expected, int32_t* loaded);
/* Name of the i-th expected weight (NULL if out of range) and its shape. */
const char* msr_weight_name(const msr_handle* h, int32_t i, int64_t* shape4, int32_t* rank);

/* ---- the generator(call) --------------------------------------------------------------------- */
/* Replaces: self.model(np.array(batch), training=False)  (process_full_tiles.py:338).
 *   in_dev   [batch, S, S, 2]  channel 0 = ortho, 1 = low-res DEM, values in [-0.5, 0.5]
 *   eps_dev  [batch, latent]   the sampler's N(0,1) draw (sampling.py:13-15); required for
 *                              MSR_GAUGAN, ignored otherwise
 *   out_dev  [batch, S, S, 1]
 * batch must equal cfg.batch_size (the reference's sampler enforces the same). */
int msr_forward(msr_handle* h, const float* in_dev, const float* eps_dev, float* out_dev, int32_t batch,
                void* stream);
/* msr_forward for callers that pipeline independent calls over two handles on two streams (the tile loop of
 * process_full_tiles.py:453-474 issues its batches one after the other; they do not depend on each other): the call's
 * latency-bound first part (encoder, dense layers, the low-resolution blocks: ~20 % of a call at low occupancy) is
 * launched at once, its matrix-bound part (from the first layer that fills the chip) waits for `gate_event`
 * (a hipEvent_t the caller recorded at the end of the previous call, on the other stream).  The heavy parts of
 * consecutive calls then run back to back and every call's head hides under its predecessor's tail — free-running
 * streams settle into either a favourable or an unfavourable phase (+6 % / -4 % against one stream), this is the
 * favourable one by construction.  gate_event == NULL: plain msr_forward.  Not captured into graphs. */
int msr_forward_gated(msr_handle* h, const float* in_dev, const float* eps_dev, float* out_dev, int32_t batch,
                      void* stream, void* gate_event);
/* on != 0: msr_forward captures its launch plan (~100 kernels on the call's stream and the handle's auxiliary stream)
 * into a HIP graph the first time it sees an (in_dev, eps_dev, out_dev) pointer triple and replays it with ONE
 * hipGraphLaunch afterwards (up to 8 triples are kept; further ones, the NULL stream and profiled calls launch
 * eagerly).  For callers that reuse their buffers — the B = 1 latency case of the serial call at
 * process_full_tiles.py:338.  Results are identical (same kernels, same order).  on == 0 drops the graphs. */
int msr_graph_enable(msr_handle* h, int32_t on);
/* Latent z [batch, latent] of the last msr_forward (debug / parity aid), copied to a device buffer. */
int msr_last_latent(msr_handle* h, float* z_dev, void* stream);

/* ---- sampler noise --------------------------------------------------------------------------- */
/* Counter-based N(0,1) noise for eps_dev of msr_forward: eps_dev[b][l] (b < B, l < L, float32, 16-byte aligned) is a pure
 * function of (seed, the id of row b, l) — not of B, of the row's position in the batch, of the stream or of earlier calls.
 * Row b's id is the three uint32 words ids_dev[3b .. 3b+2] (device memory), or (first_row + b, 0, 0) when ids_dev is NULL
 * (first_row is ignored otherwise).  Any B >= 1 and any L that is a positive multiple of 4 (B * L / 4 < 2^31), not only the
 * handle's; the handle gives the device and carries the error text.  Asynchronous on `stream`: one small kernel, no
 * allocation.  Replaces tf.random.normal (sampling.py:13) where a caller wants reproducible products: the tiler passes ids
 * that name the patch occurrence, so the noise does not depend on ranks, row windows or stream pipelining.
 *
 * The recipe is part of the ABI (a change of it is a change of MSR_ABI_VERSION).  All arithmetic after the integer block is
 * IEEE float32 with round-to-nearest + - * / and sqrt, one rounding per operation (no fused multiply-add), in exactly the
 * order written; constants are float32 values written as C hex-float literals.
 *   words    (w0, w1, w2, w3) = Philox4x32-10(counter = (l >> 2, id0, id1, id2), key = (seed & 0xFFFFFFFF, seed >> 32)),
 *            multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, 10 rounds (Random123).
 *   values   eps[b][4g + 0] = R(w0) * C(w1)    eps[b][4g + 1] = R(w0) * S(w1)          (g = l >> 2: Box-Muller, twice)
 *            eps[b][4g + 2] = R(w2) * C(w3)    eps[b][4g + 3] = R(w2) * S(w3)
 *   R(n)     = sqrt(-2 ln u), u = (n + 0.5) / 2^32:
 *            lz = leading zeros of n (32 for n = 0);  t = ((2n + 1) << lz) >> 9  (64-bit integer; 2^23 <= t < 2^24);
 *            m = float(t) * 0x1p-23;  e = -1 - lz;  if t >= 0xB504F4 { m = m * 0.5;  e = e + 1; }
 *            s = (m - 1) / (m + 1);  s2 = s * s;
 *            p = 0x1.c71c72p-4;  p = p * s2 + 0x1.24924ap-3;  p = p * s2 + 0x1.99999ap-3;  p = p * s2 + 0x1.555556p-2;
 *            p = p * s2 + 1;  ln = float(e) * 0x1.62e43p-1 + (s + s) * p;  R = sqrt(-2 * ln)
 *   C, S(n)  = cos, sin of 2 pi (n + 0.5) / 2^32:
 *            o = n >> 29;  f = n & 0x1FFFFFFF;  if o is odd { f = 0x1FFFFFFF - f; }
 *            a = float(((f >> 6) << 1) | 1) * 0x1p-24;  x = a * 0x1.921fb6p-1;  x2 = x * x;
 *            q = 0x1.71de3ap-19;  q = q * x2 - 0x1.a01a02p-13;  q = q * x2 + 0x1.111112p-7;  q = q * x2 - 0x1.555556p-3;
 *            sn = x + x * (x2 * q);
 *            r = -0x1.27e4fcp-22;  r = r * x2 + 0x1.a01a02p-16;  r = r * x2 - 0x1.6c16c2p-10;  r = r * x2 + 0x1.555556p-5;
 *            r = r * x2 - 0.5;  cs = 1 + x2 * r;
 *            (C, S) = (sn, cs) if o is 1, 2, 5 or 6, else (cs, sn);  C = -C if o is 2, 3, 4 or 5;  S = -S if o >= 4.
 * u lies in the open interval (0, 1), so every value is finite; |eps| <= sqrt(66 ln 2) = 6.77.
 * moonsuperresolution_amd.ops.sampler_noise is the NumPy twin, equal bit for bit. */
int msr_sampler_noise(msr_handle* h, uint64_t seed, const uint32_t* ids_dev, uint32_t first_row, float* eps_dev, int32_t B,
                      int32_t L, void* stream);

/* ---- tiler / stitcher ------------------------------------------------------------------------ */
/* Replaces getPatch + normalize for a whole tile (process_full_tiles.py:269-311, 453-457).
 * For every patch origin (ox[i], oy[i]) (padded-canvas coordinates, int32 on device):
 *   valid[i]   = no pixel <= no_value in either raster             (uint8)
 *   minmax[i]  = {img_min, img_max, dem_min, dem_max}               (float32 x4)
 * img_dev / dem_dev are the padded float32 rasters [rows, cols] (pitch = cols). */
int msr_patch_stats(msr_handle* h, const float* img_dev, const float* dem_dev, int32_t rows, int32_t cols,
                    const int32_t* ox_dev, const int32_t* oy_dev, int32_t n, float no_value,
                    uint8_t* valid_dev, float* minmax_dev, void* stream);
/* Writes normalised patches [n, S, S, 2] for the given origins; origin (-1,-1) = the all-zero padding
 * patch of process_full_tiles.py:468-474. */
int msr_extract_patches(msr_handle* h, const float* img_dev, const float* dem_dev, int32_t rows, int32_t cols,
                        const int32_t* ox_dev, const int32_t* oy_dev, const float* minmax_dev, int32_t n,
                        float* out_dev, void* stream);
/* Replaces the batch assembly of processTile (process_full_tiles.py:455-474: skip invalid patches, keep generation
 * order, cut into calls of `batch`, pad the last call with zero patches keyed (-1,-1)) for one tile, on the device:
 * a stable compaction of the n candidates of msr_patch_stats by their validity flags.
 *   cap           capacity of the outputs = ceil(n / batch) * batch (all-valid worst case)
 *   sel_x / sel_y [cap] int32   origins (padded-canvas coordinates) in generation order, then (-1,-1) padding:
 *                               what msr_extract_patches takes, `batch` entries per generator call
 *   sel_minmax    [cap][4]      their {img_min, img_max, dem_min, dem_max}; zeros for padding
 *   key           [cap][2]      origins relative to (tile_x, tile_y) = the reference's dict keys; (-1,-1) padding
 *   dmm           [cap][2]      {dem_min, dem_max}: what msr_stitch_tile takes
 *   meta          [2] int32     {number of valid patches, number of generator calls}
 * The host reads back only `meta` (8 bytes). */
int msr_compact_patches(msr_handle* h, const uint8_t* valid_dev, const int32_t* ox_dev, const int32_t* oy_dev,
                        const float* minmax_dev, int32_t n, int32_t tile_x, int32_t tile_y, int32_t batch, int32_t cap,
                        int32_t* sel_x_dev, int32_t* sel_y_dev, float* sel_minmax_dev, int32_t* key_dev,
                        float* dmm_dev, int32_t* meta_dev, void* stream);
/* msr_compact_patches for a caller that carries the unfilled tail of one compaction into the next (the halo mode's
 * batching="rank": a rank's valid patches form ONE sequence cut at multiples of `batch`, whatever the bands it is generated
 * in).  Slots [0, carry_n) of the five output arrays are the caller's: it copies the carried rows there (device to device)
 * and the kernel leaves them untouched.  The stable compaction starts at slot carry_n, the (-1,-1) padding runs from
 * carry_n + valid to cap, and meta = {carry_n + valid, ceil((carry_n + valid) / batch)}.
 * carry_n outside [0, batch) or cap < ceil((carry_n + n) / batch) * batch is MSR_ERR_INVALID before anything is launched. */
int msr_compact_patches_carry(msr_handle* h, const uint8_t* valid_dev, const int32_t* ox_dev, const int32_t* oy_dev,
                              const float* minmax_dev, int32_t n, int32_t tile_x, int32_t tile_y, int32_t batch, int32_t cap,
                              int32_t carry_n, int32_t* sel_x_dev, int32_t* sel_y_dev, float* sel_minmax_dev,
                              int32_t* key_dev, float* dmm_dev, int32_t* meta_dev, void* stream);
/* Replaces processBatch's "+0.5" and rebuildTile (process_full_tiles.py:340, 363-414) for one tile.
 *   pred_dev    [n, S, S]  generator outputs (last channel), in generation order
 *   key_dev     [n, 2]     int32 (x, y) of each patch relative to the tile origin (padded coords)
 *   dmm_dev     [n, 2]     float32 (dem_min, dem_max) of each patch
 *   mean/std    [T, T] float32, good [T, T] uint8
 * as_implemented != 0 reproduces the reference's aliased variance update. */
int msr_stitch_tile(msr_handle* h, const float* pred_dev, const int32_t* key_dev, const float* dmm_dev, int32_t n,
                    int32_t tile_size, int32_t stride, float no_value, int32_t as_implemented,
                    float* mean_dev, float* std_dev, uint8_t* good_dev, void* stream);

/* ---- patch-row-sharded ("halo") mode: north_star's exchange of overlap halos (second mode) ------------
 * The reference has no counterpart: it re-generates the halo patches of every tile (process_full_tiles.py:449-454).
 * msr_stitch_partial is msr_stitch_tile stopped before the finalisation of :409-413, with the textbook (West) variance
 * update: it returns the raw accumulators (w_sum, mean, S) [T, T] of the patches it was given, so that two ranks that
 * each hold part of the patches covering a pixel can combine them. */
int msr_stitch_partial(msr_handle* h, const float* pred_dev, const int32_t* key_dev, const float* dmm_dev, int32_t n,
                       int32_t tile_size, int32_t stride, float* wsum_dev, float* mean_dev, float* s_dev, void* stream);
/* msr_stitch_partial writing IN PLACE into a T x T window of larger accumulator images (row pitch `pitch` >= tile_size
 * elements) and, with resume != 0, continuing the running update from what the window already holds instead of from zero:
 * the banded form of the halo mode (moonsuperresolution_amd/halo.py) — a rank generates its patch rows band by band (in
 * generation order), accumulates each band into the canvas rows it reaches and frees its predictions.  The sequence of
 * updates per pixel is the all-at-once sequence, so the STITCHER does not depend on the band size, bit for bit, given
 * identical predictions.  The predictions of a model with batch statistics (SPADE) depend on their batch mates: they are
 * independent of the bands only when the batches are (halo.py, batching="rank": msr_compact_patches_carry). */
int msr_stitch_accumulate(msr_handle* h, const float* pred_dev, const int32_t* key_dev, const float* dmm_dev, int32_t n,
                          int32_t tile_size, int32_t stride, float* wsum_dev, float* mean_dev, float* s_dev, int32_t pitch,
                          int32_t resume, void* stream);
/* The same accumulation for a whole band in one pass, instead of one msr_stitch_accumulate per T x T block: one thread per
 * pixel of canvas rows [row_lo, row_hi) x [0, width) of an accumulator slab whose row 0 / column 0 the three pointers name
 * (row pitch `pitch` >= width elements, row 0 = canvas row acc_row0 <= row_lo).  key_dev holds CANVAS origins (what
 * msr_compact_patches writes with tile_x = tile_y = 0); the band's patch grid is ngx x ngy cells, cell (0, 0) at canvas
 * origin (grid_x0, grid_y0), cells `stride` apart; grid_ws_dev is a caller-provided int32 workspace of ngx * ngy cells.
 * Origins off the grid or not on the stride are ignored.  Every pixel resumes from the slab, applies the updates of the
 * patches covering it (y outer, x inner) and writes back: the bits msr_stitch_accumulate(resume = 1) leaves over the blocks.
 * Null pointers, pitch < width, an empty or inverted row range, row_lo < acc_row0 and a non-positive grid are
 * MSR_ERR_INVALID before anything is launched. */
int msr_stitch_accumulate_band(msr_handle* h, const float* pred_dev, const int32_t* key_dev, const float* dmm_dev, int32_t n,
                               int32_t stride, int32_t grid_x0, int32_t grid_y0, int32_t ngx, int32_t ngy,
                               int32_t* grid_ws_dev, float* wsum_dev, float* mean_dev, float* s_dev, int32_t pitch,
                               int32_t acc_row0, int32_t row_lo, int32_t row_hi, int32_t width, void* stream);
/* Pairwise (Chan) combine of two sets of accumulators of the same `count` pixels — a = the rank with the earlier patch
 * rows, b = the later one, or b == NULL — followed by rebuildTile's finalisation (good = w_sum > 0,
 * std = sqrt(S / w_sum), no_value where not good; process_full_tiles.py:409-413). */
int msr_halo_merge(msr_handle* h, const float* wa_dev, const float* ma_dev, const float* sa_dev, const float* wb_dev,
                   const float* mb_dev, const float* sb_dev, int64_t count, float no_value, float* mean_dev,
                   float* std_dev, uint8_t* good_dev, void* stream);

/* Optional: replace the library's own blending window (makeGaussianKernel + 1e-7, purged S//16 per side,
 * process_full_tiles.py:347-361,391-393) by a caller-computed float64 [S-2p, S-2p] HOST array — the Python
 * host passes NumPy's own evaluation so the GPU stitcher is bit-identical to the NumPy reference. */
int msr_set_blend_window(msr_handle* h, const double* host_window, int32_t side);

/* CRC-32C (Castagnoli) of a HOST buffer, continuing from `crc` (0 to start).  Host-only helper of the TensorBundle
 * weight reader (moonsuperresolution_amd/tf_checkpoint.py): checkpoint data and index blocks carry masked CRC-32C. */
uint32_t msr_crc32c(const void* host_data, uint64_t n, uint32_t crc);

/* ---- pre-processing resamplers ------------------------------------------------ */
/* Replaces cv2.resize(dem, (0,0), fx=1/factor, fy=1/factor, interpolation=cv2.INTER_AREA) of preprocess
 * (process_full_tiles.py:232,238) on a float32 raster [rows, cols] in device memory: dst [dst_rows, dst_cols] with
 * dst_* = cvRound(src_* / factor); every destination pixel is the mean of its factor x factor block (NaN propagates;
 * partial edge blocks average the pixels that exist). */
int msr_resize_area(msr_handle* h, const float* src_dev, int32_t rows, int32_t cols, int32_t factor, float* dst_dev,
                    int32_t dst_rows, int32_t dst_cols, void* stream);
/* Replaces cv2.resize(dem_rs, dsize, interpolation=cv2.INTER_CUBIC) (process_full_tiles.py:241): Keys cubic,
 * A = -0.75, pixel-centre mapping, replicated border, float32; dst [dst_rows, dst_cols]. */
int msr_resize_cubic(msr_handle* h, const float* src_dev, int32_t rows, int32_t cols, float* dst_dev,
                     int32_t dst_rows, int32_t dst_cols, void* stream);
/* The same two resamplers on ROW WINDOWS, for a process that holds only some rows of a raster (a rank of a sharded run:
 * moonsuperresolution_amd/preprocess.py::preprocess_rows).  src_dev holds rows [src_row0, src_row0 + src_rows) of a source of
 * full_rows (full_src_rows) x cols; dst_dev receives rows [dst_row0, dst_row0 + dst_rows) of the whole-raster result, all
 * dst_cols columns, and holds the bits msr_resize_area / msr_resize_cubic write to those rows: block geometry, partial edge
 * blocks, the cubic's scale (full_src_rows / full_dst_rows) and its border clamp come from the full sizes, and only the final
 * source row index is rebased by src_row0.  A window that lacks a source row one of the destination rows reads is
 * MSR_ERR_INVALID (the message names the rows) before anything is launched.
 * flags fuse the no-data marking of preprocess (process_full_tiles.py:231,233,237,242) into the pass:
 *   MSR_RESIZE_NODATA_TO_NAN   a source value <= no_value is read as NaN
 *   MSR_RESIZE_NAN_TO_NODATA   a NaN result is stored as no_value */
#define MSR_RESIZE_NODATA_TO_NAN 1
#define MSR_RESIZE_NAN_TO_NODATA 2
int msr_resize_area_rows(msr_handle* h, const float* src_dev, int32_t src_row0, int32_t src_rows, int32_t full_rows,
                         int32_t cols, int32_t factor, float* dst_dev, int32_t dst_row0, int32_t dst_rows, int32_t dst_cols,
                         float no_value, int32_t flags, void* stream);
int msr_resize_cubic_rows(msr_handle* h, const float* src_dev, int32_t src_row0, int32_t src_rows, int32_t full_src_rows,
                          int32_t cols, float* dst_dev, int32_t dst_row0, int32_t dst_rows, int32_t full_dst_rows,
                          int32_t dst_cols, float no_value, int32_t flags, void* stream);

/* ---- pre-processing: in-filling of small no-data holes (preprocess(infill="device")) ---------------------------------
 * Fills, in place, the small holes of a float32 grid in DEVICE memory (csrc/infill.hip, csrc/infill_solve.h).  It stands in
 * for fillNan / interpolateMissingValues of the reference (process_full_tiles.py:184-224) with a stated deviation: the SAME
 * pixels are filled, with other values (a local thin-plate fill in place of griddata's cubic surface).  The NumPy twin
 * moonsuperresolution_amd/infill.py::infill_reference defines the result; the kernels equal it bit for bit.
 *
 * grid_dev holds rows [row0, row0 + n_rows) of a grid of full_rows x cols.
 *   hole       a pixel with !(G[p] > no_value); NaN is a hole.  Outside the window there are neither holes nor valid pixels.
 *   component  an 8-connected set of holes.
 *   fill set F every hole whose component has fewer than max_area pixels and that lies margin <= row < full_rows - margin,
 *              margin <= col < cols - margin in whole-grid coordinates and, where the window is cut (row0 > 0, or
 *              row0 + n_rows < full_rows), at least max_area rows from the cut.
 *   unknowns   for each component K that meets F: the pixels of K in row-major order.
 *   centres    K and the 4-neighbours of K; a centre is used iff each of its five stencil pixels is in K or is valid.  Every
 *              pixel of K is a used centre, so the system below is positive definite.
 *   equation   per used centre: -4 u(centre) + the sum of u over its four neighbours = 0, valid pixels on the right.
 *   solution   the least-squares solution, by the normal equations in float64 and a Cholesky factorisation without
 *              pivoting; csrc/infill_solve.h states the order of every sum.
 *   result     rounded once to float32 and stored at K ∩ F.  Every other element of the grid keeps its bits.
 * A window writes, at every row at least max_area rows from its cut edges, the bits the whole grid gets, and nothing at the
 * other rows.  Only positions relative to a component enter its solution.
 * preprocess uses (max_area, margin) = (24, 32) on the x1/4 grid and (8, 128) on the ortho: fillNan's border and
 * max_fill_area, whose tiled census this rule reproduces.
 * workspace_dev: msr_infill_workspace_bytes(n_rows, cols) bytes of device memory, 8-byte aligned, contents irrelevant
 * (16 + 8 n_rows ceil(cols / 64) + 4 ceil(n_rows / 2) ceil(cols / 2); -1 for non-positive sizes or more than 2^31 - 1 pixels).
 * h may be NULL.  MSR_ERR_INVALID, with a message that names the argument, before any launch: a null pointer, non-positive
 * n_rows / full_rows / cols, max_area outside [2, 32], margin < max_area + 1, a window outside the grid, more than 2^31 - 1
 * pixels in the window, a workspace that is too small or misaligned.  Asynchronous on `stream`; no allocation. */
int64_t msr_infill_workspace_bytes(int32_t n_rows, int32_t cols);
int msr_infill_small_holes(msr_handle* h, float* grid_dev, int32_t row0, int32_t n_rows, int32_t full_rows, int32_t cols,
                           float no_value, int32_t max_area, int32_t margin, void* workspace_dev, int64_t workspace_bytes,
                           void* stream);
/* One stage of msr_infill_small_holes on its own, for timing: stage 1 labels (hole bitmap and component list into the
 * workspace), stage 2 solves and stores what a stage 1 on the same arguments left there. */
int msr_debug_infill_stage(msr_handle* h, float* grid_dev, int32_t row0, int32_t n_rows, int32_t full_rows, int32_t cols,
                           float no_value, int32_t max_area, int32_t margin, void* workspace_dev, int64_t workspace_bytes,
                           void* stream, int32_t stage);
/* HOST code: the build-and-solve of ONE component (csrc/infill_solve.h, run with one lane), so that it can be checked against
 * the twin without a GPU.  grid is rows x cols host float32; (pix_r[i], pix_c[i]), i < n, are the pixels of a whole component
 * in row-major order, 1 <= n <= 31, none on the grid's outermost pixels; out[i] receives the float32 fill of pixel i.  0, or -1
 * for a null pointer, an n outside [1, 31], a pixel outside the grid's interior or out of order, or a component wider or
 * taller than 31. */
int32_t msr_infill_component_host(const float* grid, int32_t rows, int32_t cols, float no_value, const int32_t* pix_r,
                                  const int32_t* pix_c, int32_t n, float* out);

/* TIFF 6.0 LZW (compression 5) of HOST buffers, for the GeoTIFF reader / writer (moonsuperresolution_amd/geotiff.py;
 * the reference reads and writes LZW GeoTIFFs through GDAL: process_full_tiles.py:158-182, 481-531).
 * Both return the number of bytes produced, or -1 on a malformed stream / too small output buffer. */
int64_t msr_lzw_decode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t n_out);
int64_t msr_lzw_encode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);
/* The stream both encoders write, byte for byte the same for the same input bytes: ClearCode (256) first; codes MSB-first,
 * 9 to 12 bits wide; first free code 258; the width grows one code early, when the next free code reaches 512 / 1024 /
 * 2048; a ClearCode and a fresh table when it reaches 4095; after the last code the next free code advances once more (the
 * decoder adds an entry for it) with the same width rule, then EndOfInformation (257); the last byte is padded with zero
 * bits.  An empty input is ClearCode, EndOfInformation.  Matching is greedy longest-match, so the stream is canonical.
 *
 * TIFF LZW of n_strips independent strips in DEVICE memory, one launch (csrc/geotiff_codec.hip; geotiff.py
 * write_geotiff(encoder="device")).  Strip i is src_len[i] bytes at src_dev + src_off[i]; its stream goes to
 * dst_dev + dst_off[i], and dst_len[i] is the stream's byte count, or -1 when that exceeds dst_cap[i] (or src_len[i] < 0).
 * No byte at or beyond dst_off[i] + dst_cap[i] is written; the slots must not overlap.  All five arrays are device memory.
 * sample_bytes 0: the bytes are encoded as they are.  1, 2 or 4: the TIFF horizontal predictor (PREDICTOR=2) is applied on
 * the fly to little-endian samples of that width, restarting every row_bytes (a positive multiple of sample_bytes): a strip
 * holds whole rows, the first sample of a row passes through, the others become u[j] - u[j-1] modulo the sample width.
 * src is not modified.  h may be NULL (the codec keeps no handle state; errors then go to msr_last_error(NULL)).
 * MSR_ERR_INVALID before any launch for a null pointer, n_strips < 0, a sample_bytes outside {0, 1, 2, 4} or a row_bytes that
 * is not a positive multiple of a non-zero sample_bytes.  Asynchronous on `stream`; no allocation. */
int msr_lzw_encode_strips(msr_handle* h, const uint8_t* src_dev, const int64_t* src_off_dev, const int32_t* src_len_dev,
                          int32_t n_strips, int32_t sample_bytes, int32_t row_bytes,
                          uint8_t* dst_dev, const int64_t* dst_off_dev, const int32_t* dst_cap_dev, int32_t* dst_len_dev,
                          void* stream);
/* The same streams for n_blocks blocks (tiles) read IN PLACE from row-major rasters in DEVICE memory, one launch, one block per
 * one-wave workgroup (grid-stride): no padded frame and no tile-major copy is needed (geotiff.py write_geotiff(layout="cog",
 * encoder="device")).  A block is block_h rows of block_w_bytes bytes.  Byte q of block i is row y = q / block_w_bytes, column
 * byte x = q % block_w_bytes: src_dev[blk_off[i] + y * blk_pitch[i] + x] where y < blk_rows[i] and x < blk_wbytes[i] (the
 * valid part: what of the block lies in the raster), zero elsewhere (the padding of an edge tile).  blk_off is the byte offset
 * of the block's first sample, blk_pitch the bytes between raster rows of the block's level: it is per block, so blocks of
 * several levels, each row-major at its own pitch in one allocation, share a launch.  All offset arithmetic is 64-bit.
 * sample_bytes as above, with the padding in place BEFORE the predictor, which restarts on every block row: the first padding
 * sample of a row is 0 - the last valid sample.  The stream of block i is msr_lzw_encode of those block_w_bytes * block_h
 * bytes, byte for byte; dst_off / dst_cap / dst_len as above, and dst_len[i] = -1 too where blk_wbytes[i] is outside
 * [0, block_w_bytes] or blk_rows[i] outside [0, block_h].  The caller keeps every valid part inside src (geotiff.py checks it
 * on the host).  All seven arrays are device memory.  h may be NULL.  MSR_ERR_INVALID before any launch, with a message that
 * names the argument: a null pointer, n_blocks < 0, a sample_bytes outside {0, 1, 2, 4}, a block_w_bytes that is not a positive
 * multiple of sample_bytes (of 1 for 0), block_h <= 0, a block of more than 2^30 bytes.  n_blocks == 0 is MSR_OK without a
 * launch.  Asynchronous on `stream`; no allocation. */
int msr_lzw_encode_blocks(msr_handle* h, const uint8_t* src_dev, const int64_t* blk_off_dev, const int64_t* blk_pitch_dev,
                          const int32_t* blk_wbytes_dev, const int32_t* blk_rows_dev, int32_t n_blocks, int32_t block_w_bytes,
                          int32_t block_h, int32_t sample_bytes, uint8_t* dst_dev, const int64_t* dst_off_dev,
                          const int32_t* dst_cap_dev, int32_t* dst_len_dev, void* stream);
/* HOST code: the function msr_lzw_encode_blocks runs for one block (csrc/lzw_strip.h: the in-place fetch and the automaton),
 * run with one lane on host buffers, so that it can be checked against msr_lzw_encode of the padded, differenced block
 * without a GPU.  The block's first sample is at src.  Returns the stream's length, or -1 when it exceeds cap (no byte at or
 * beyond dst + cap is written) and for an argument msr_lzw_encode_blocks rejects, a valid part outside the block, or a cap
 * that is negative or above INT32_MAX. */
int64_t msr_lzw_encode_block_host(const uint8_t* src, int64_t pitch, int32_t valid_w_bytes, int32_t valid_rows,
                                  int32_t block_w_bytes, int32_t block_h, int32_t sample_bytes, uint8_t* dst, int64_t cap);
/* The three entries above with the TIFF Predictor tag's value given beside the samples' width: sample_bytes is 1, 2 or 4 and
 * predictor 1, 2 or 3; row_bytes / block_w_bytes is a positive multiple of sample_bytes whatever the predictor.  Everything not
 * said here is as above: the arrays, the slots, dst_len, the stream rules, the further argument checks, the return values.
 * predictor 1: the bytes as they are, byte for byte the entries above with sample_bytes 0.  predictor 2: the horizontal
 * predictor, byte for byte the entries above with this sample_bytes.  predictor 3: the floating-point predictor of TIFF
 * Technical Note 3 for little-endian float32 samples, which needs sample_bytes 4.  Every row of w = row_bytes / 4 samples
 * (every block row, w = block_w_bytes / 4) is regrouped into four planes, the most significant byte of every sample first:
 * regrouped byte q = p * w + x is T(q) = byte 3 - p of sample x.  Then every byte but the row's first is differenced over the
 * whole regrouped row, across the plane boundaries: the encoder sees T(0), T(1) - T(0), ..., T(4w - 1) - T(4w - 2) modulo 256
 * (libtiff's fpDiff with stride 1; geotiff.py fp_predictor_reference is the NumPy twin).  A strip holds whole rows.  In a block
 * the padding is in place BEFORE the predictor and the predictor restarts on every block row; a sample that does not lie whole
 * inside the valid part (inside the strip's src_len bytes) is padding, so blk_wbytes is meant to be a multiple of 4; row offsets
 * are y * blk_pitch in 64-bit.  Rows that start on a 4-byte boundary are read with aligned 32-bit loads, others byte by byte;
 * the stream is the same.  MSR_ERR_INVALID before any launch, with a message that names the argument, also for a predictor
 * outside {1, 2, 3}, a sample_bytes outside {1, 2, 4}, and predictor 3 with another sample_bytes than 4;
 * msr_tiff_encode_block_host returns -1 for these.  The read-side counterpart is the host reader (geotiff.py read_geotiff):
 * msr_tiff_blocks_to_f32 undoes predictors 1 and 2 only. */
int msr_tiff_encode_strips(msr_handle* h, const uint8_t* src_dev, const int64_t* src_off_dev, const int32_t* src_len_dev,
                           int32_t n_strips, int32_t sample_bytes, int32_t predictor, int32_t row_bytes,
                           uint8_t* dst_dev, const int64_t* dst_off_dev, const int32_t* dst_cap_dev, int32_t* dst_len_dev,
                           void* stream);
int msr_tiff_encode_blocks(msr_handle* h, const uint8_t* src_dev, const int64_t* blk_off_dev, const int64_t* blk_pitch_dev,
                           const int32_t* blk_wbytes_dev, const int32_t* blk_rows_dev, int32_t n_blocks, int32_t block_w_bytes,
                           int32_t block_h, int32_t sample_bytes, int32_t predictor, uint8_t* dst_dev, const int64_t* dst_off_dev,
                           const int32_t* dst_cap_dev, int32_t* dst_len_dev, void* stream);
int64_t msr_tiff_encode_block_host(const uint8_t* src, int64_t pitch, int32_t valid_w_bytes, int32_t valid_rows,
                                   int32_t block_w_bytes, int32_t block_h, int32_t sample_bytes, int32_t predictor, uint8_t* dst,
                                   int64_t cap);

/* The reverse: n_strips independent TIFF LZW blocks (strips or tiles) in DEVICE memory decoded in one launch, one block per
 * one-wave workgroup (csrc/geotiff_codec.hip, csrc/lzw_unstrip.h; geotiff.py read_geotiff(decoder="device")).  Block i is
 * src_len[i] bytes at src_dev + src_off[i]; its bytes go to dst_dev + dst_off[i], and dst_len[i] is what
 * msr_lzw_decode(block i, src_len[i], slot i, dst_cap[i]) returns, with the same bytes [0, dst_len[i]), for every input,
 * well-formed or not.  The stream rules: codes MSB-first, 9 to 12 bits wide; 256 is ClearCode and may come anywhere (twice in a
 * row, or not at the start); 257 is EndOfInformation, bytes after it are ignored; first free code 258; the width grows when the
 * next free code reaches 511 / 1023 / 2047; no entry is added once it is 4096 and codes stay 12 bits wide; the first code
 * after a Clear adds no entry; a code equal to the next free code is the KwKwK case; a code above it, or a code >= 256 right
 * after a Clear, gives -1; so does an output longer than dst_cap[i] and a negative src_len[i] or dst_cap[i]; a stream that ends
 * without EndOfInformation gives the bytes produced so far.  In addition, 0 <= dst_len[i] < dst_cap[i] zeroes bytes
 * [dst_len[i], dst_cap[i]) of the slot.  No byte at or beyond dst_off[i] + dst_cap[i] is written; the slots must not overlap.
 * All five arrays are device memory.  h may be NULL.  MSR_ERR_INVALID before any launch for a null pointer or n_strips < 0;
 * n_strips == 0 is MSR_OK without a launch.  Asynchronous on `stream`; no allocation. */
int msr_lzw_decode_strips(msr_handle* h, const uint8_t* src_dev, const int64_t* src_off_dev, const int32_t* src_len_dev,
                          int32_t n_strips, uint8_t* dst_dev, const int64_t* dst_off_dev, const int32_t* dst_cap_dev,
                          int32_t* dst_len_dev, void* stream);
/* Decoded TIFF blocks in DEVICE memory -> a float32 raster window, one launch: undoes the horizontal predictor, converts and
 * places.  Block i is block_h rows of block_w little-endian samples (sample_kind 'u' / 'i' / 'f', sample_bytes 1, 2 or 4; float
 * needs 4) at src_dev + blk_off[i], and its first sample is raster pixel (blk_x0[i], blk_y0[i]).  out_dev is
 * [out_rows, cols] float32 whose first row is raster row out_row0.  For every block row inside the window: with predictor 2 the
 * samples become the running sum along the row modulo the sample width (on the unsigned bit pattern, restarting at every block
 * row: the bits of NumPy's cumsum on the unsigned view), with predictor 1 they are taken as they are; then (float) of the
 * integer, float32 passing through bit for bit (NaN payloads included); columns [x0, min(x0 + block_w, cols)) are written.
 * Rows outside the window and columns outside the raster are never written, and block rows outside the window are never
 * read (a short last strip may end with the raster).  h may be NULL.  MSR_ERR_INVALID before any launch for a null pointer,
 * n_blocks < 0, an unknown kind or width, a predictor other than 1 or 2, or block_w, block_h, out_rows, cols <= 0 or
 * out_row0 < 0; n_blocks == 0 is MSR_OK without a launch.  Asynchronous on `stream`; no allocation. */
int msr_tiff_blocks_to_f32(msr_handle* h, const uint8_t* src_dev, const int64_t* blk_off_dev, const int32_t* blk_x0_dev,
                           const int32_t* blk_y0_dev, int32_t n_blocks, int32_t block_w, int32_t block_h, int32_t sample_kind,
                           int32_t sample_bytes, int32_t predictor, float* out_dev, int32_t out_row0, int32_t out_rows,
                           int32_t cols, void* stream);
/* HOST code: the automaton msr_lzw_decode_strips runs on the device (csrc/lzw_unstrip.h), run with one lane on host buffers, so
 * that it can be checked against msr_lzw_decode without a GPU.  The result and the bytes are msr_lzw_decode's, plus the zeroed
 * tail [result, cap); -1 for a null pointer, a negative argument or one above INT32_MAX. */
int64_t msr_lzw_decode_strip_host(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);

/* One reduced-resolution level (a TIFF overview) of a raster in DEVICE memory, one launch (csrc/tiff_overview.hip, the rule in
 * csrc/tiff_overview.h; geotiff.py write_geotiff(tile=, overviews=, encoder="device"), twin: geotiff.overview_reference).
 * src_dev is [rows, cols] samples of sample_kind 'f' (sample_bytes 4: float32) or 'u' (sample_bytes 1 or 2), dst_dev
 * [ceil(rows / 2), ceil(cols / 2)] of the same type.  dst[i][j] comes from src[2i : 2i + 2][2j : 2j + 2] clipped to the raster.
 *   float32  a pixel counts iff v != no_value (a NaN counts and propagates; has_nodata = 0: every pixel counts).  No counting
 *            pixel: no_value.  Otherwise s / (float)n, s the float32 sum of the n counting values in row-major order started
 *            from the first of them, not from 0 (-0.0 alone stays -0.0): one rounding per addition and one for the division.
 *   uint     the maximum of the block.
 * One thread per destination pixel, 64-bit offsets, no LDS.  src is not modified; src and dst must not overlap.  h may be NULL.
 * MSR_ERR_INVALID before any launch, with a message that names the argument: a null pointer, rows or cols <= 0, more than
 * 2^31 - 1 source pixels, an unknown kind or width, has_nodata other than 0 / 1 or set with an integer kind.  Asynchronous on
 * `stream`; no allocation. */
int msr_overview_half(msr_handle* h, const void* src_dev, int32_t rows, int32_t cols, int32_t sample_kind, int32_t sample_bytes,
                      int32_t has_nodata, float no_value, void* dst_dev, void* stream);
/* HOST code: the same rule (the same function of csrc/tiff_overview.h) looped over host buffers, so that it can be checked
 * against the twin without a GPU.  0, or -1 for an argument msr_overview_half rejects. */
int msr_overview_half_host(const void* src, int32_t rows, int32_t cols, int32_t sample_kind, int32_t sample_bytes,
                           int32_t has_nodata, float no_value, void* dst);

/* ---- measurement ----------------------------------------------------------------------------- */
typedef struct {
    char name[48];        /* kernel family, e.g. "conv_igemm_f32" */
    int64_t launches;
    double device_ms;     /* sum of hipEvent-bracketed launch durations on the call's stream */
    double flops;         /* algorithmic FLOPs of those launches (2*MACs), 0 for memory-bound families */
    double bytes;         /* algorithmic bytes of those launches */
} msr_kernel_stat;
/* on = 1: every kernel launch of msr_forward is bracketed by hipEvents on the call's stream (an event costs the
 * stream 2-3 us: ~7 % of a call's throughput).  on = 2: only the conv family is timed and a run of consecutive conv
 * launches shares one pair of events (device_ms then includes the 1.5-3 us gaps inside a run; < 2 % overhead).
 * on = 0: off. */
int msr_profile_enable(msr_handle* h, int32_t on);
int msr_profile_reset(msr_handle* h);
/* Synchronises the recorded events and fills up to cap entries; *n = number of families. */
int msr_profile_read(msr_handle* h, msr_kernel_stat* out, int32_t cap, int32_t* n);
/* The recorded intervals of one family (0 = the conv family), in ms relative to ref_event (a hipEvent_t the caller
 * recorded before the calls): lets a caller that drives several handles on several streams take the UNION of the
 * family's busy intervals instead of their sum. */
int msr_profile_runs(msr_handle* h, void* ref_event, int32_t family, double* start_ms, double* end_ms, double* flops,
                     int64_t* launches, int32_t cap, int32_t* n);
/* Algorithmic FLOPs of one msr_forward call (all patches), the figure BASELINE.md section 2 derives. */
int msr_forward_flops(const msr_handle* h, double* flops);
/* Kernel-level entry (parity tests and micro-benchmarks of the dominant kernel): one conv_igemm_f32 launch.
 *   in_dev   zero-bordered NHWC input [B, rin+2, rin+2, Cin], rin = rout*stride
 *   wt_dev   weights already in the kernel layout [9][N][Cin]; bias_dev [N] (GEMM column order)
 *   epilogue 0 bias, 1 bias+residual(aux [B, rout>>aux_shift, ., N]), 2 SPADE (N = 2C, interleaved columns;
 *            aux = x [B, rout>>aux_shift, ., C], mean/std [C]); out_padded != 0 writes a zero-bordered tensor
 *   tile     -1 auto (tile and K split chosen by the library), else (0 = 128x128 | 1 = 64x64) + 256 * ksplit */
int msr_op_conv3x3(msr_handle* h, const float* in_dev, const float* wt_dev, const float* bias_dev, float* out_dev,
                   int32_t B, int32_t rout, int32_t Cin, int32_t N, int32_t stride, int32_t epilogue,
                   const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev,
                   int32_t out_padded, int32_t tile, void* stream);
/* Kernel-level entry of the plain fp32 conv with explicit geometry and the affine epilogue (EPI_AFFINE), as the pix2pix plan
 * launches it: out = act(conv(in, wt) * scale[c] + shift[c]), one conv_igemm_f32 launch (plus the split-K pass for ksplit > 1).
 *   in_dev    pointer to tap (0, 0), channel 0 of output pixel (0, 0) of sample 0: output (b, y, x) reads, for tap (kh, kw) and
 *             channel k < Cin, in_dev[b * in_pb + (y * stride + kh) * in_py + (x * stride + kw) * in_px + k].  in_px > Cin reads a
 *             channel slice of a wider buffer; a caller realises 'same' padding with a zero border, and a parity of a transposed conv
 *             by advancing in_dev.  Pitches in floats, multiples of 4
 *   wt_dev    [KH * KW][N][Cin];  scale_dev [N] or NULL (= 1);  shift_dev [N]
 *   out_dev   output (b, y, x), channel c < N goes to out_dev[out_off + b * out_pb + y * out_py + x * out_px + c]: out_px > N
 *             writes one half of a concat buffer, out_px = 2 * (channels per pixel) every second pixel.  Nothing else is written
 *   rout      output side, a power of two;  Cin % 32 == 0;  N % 64 == 0 (% 128 on the 128 x 128 tile);  stride 1 | 2
 *   act       0 none, 1 relu, 2 leaky_relu(slope)
 *   tile      -1 auto (the planner's conv_form), else (0 = 128x128 | 1 = 64x64) + 256 * ksplit (0 or 1 = whole K; at most
 *             KH * KW * Cin / 32 ranges)
 * A shape the kernel has no instantiation for, a misaligned pointer or pitch, and tensors beyond 2^31 elements are MSR_ERR_INVALID
 * with a message, checked before anything touches the device: h may be NULL for that (the text is msr_last_error(NULL)); with valid
 * arguments a NULL handle is MSR_ERR_INVALID too.  Asynchronous on `stream`. */
int msr_op_conv_affine(msr_handle* h, const float* in_dev, int32_t in_px, int32_t in_py, int32_t in_pb, const float* wt_dev,
                       const float* scale_dev, const float* shift_dev, float* out_dev, int32_t out_off, int32_t out_px,
                       int32_t out_py, int32_t out_pb, int32_t B, int32_t rout, int32_t Cin, int32_t N, int32_t KH, int32_t KW,
                       int32_t stride, int32_t act, float slope, int32_t tile, void* stream);
/* The same with in_dev / wt_dev holding split-bf16 words (msr_op_split_bf16) and the bf16x3 arithmetic;
 * out_split != 0 (SPADE epilogue only) writes split-bf16 words too.  tile: (0 = 128x128 | 1 = 64x64 | 3, 4 = LDS-halo
 * forms | 5 = persistent ping-pong) + 0x40 (weights in MFMA-fragment order, tiles 0 / 1) + 0x80 (tile 5, SPADE epilogue
 * only: in_dev / wt_dev hold split-FP16 words and the products are the 2-term form of MSR_FLAG_GB_F16X2) + 256 * ksplit. */
int msr_op_conv3x3_bf16x3(msr_handle* h, const float* in_dev, const float* wt_dev, const float* bias_dev,
                          float* out_dev, int32_t B, int32_t rout, int32_t Cin, int32_t N, int32_t stride,
                          int32_t epilogue, const float* aux_dev, int32_t aux_shift, const float* mean_dev,
                          const float* std_dev, int32_t out_padded, int32_t out_split, int32_t tile, void* stream);
/* Kernel-level entry of the f16c form (MSR_FLAG_F16C) of the persistent ping-pong conv: in_dev / wt_dev hold f16c chunk
 * images (moonsuperresolution_amd.ops.f16c_activation_image / f16c_weight_image restate the format), wexp_dev [N] =
 * (127 + e_lo) | (127 + e_hi) << 8; out_mode (SPADE epilogue) 0 = fp32, 1 = split-bf16 words, 4 = f16c image, 5 = f16c6 image,
 * plus in its high bits:
 *   + 256 * ksplit   K ranges (ksplit a power of two dividing Cin / 64; 0 or 1 = whole tiles): the ping-pong kernel writes raw
 *                    accumulators to the handle's split-K workspace and a second pass applies the epilogue (out_mode 0, 1, 4),
 *                    as the planner launches layers with fewer tiles than CUs
 *   + 0x10000        no cross terms (MSR_FLAG_F16_MAIN's form: x_hi * w_hi only) on the stream kernel; whole tiles, bias /
 *                    residual epilogue, Cin % 128 == 0, power-of-two rout only
 * Anything else is MSR_ERR_INVALID. */
int msr_op_conv3x3_f16c(msr_handle* h, const float* in_dev, const float* wt_dev, const int32_t* wexp_dev,
                        const float* bias_dev, float* out_dev, int32_t B, int32_t rout, int32_t Cin, int32_t N,
                        int32_t epilogue, const float* aux_dev, int32_t aux_shift, const float* mean_dev,
                        const float* std_dev, int32_t out_padded, int32_t out_mode, void* stream);
/* Kernel-level entry of conv_gb_resident (csrc/conv_gbr.hip): ONE SPADE layer's modulation path in one launch —
 *   nearest resize of src to r x r + Conv2D(128, 3, relu) (spade.py:17-18), conv_gamma | conv_beta (spade.py:19-20) as one
 *   GEMM with N = 2C columns interleaved (32 gamma | 32 beta), gamma * (x - mean) / std + beta (spade.py:21-24), leaky_relu(0.2)
 *   (blocks.py:30-34), written as the f16c chunk image of the consumer conv.
 *   src_dev  [B, S, S, 2] fp32 (S = r * 2^k); we_dev HWIO [3,3,2,128]; be_dev [128]
 *   wt_dev   the kernel's weight stream (ops.gbr_weight_image restates it): the f16c6 image of [9][N][128] with the input
 *            channels of every 32-chunk in position order (position e holds channel 8 * (e >> 3) + 4 * (e & 1) + ((e >> 1) & 3)),
 *            re-ordered into [channel block][wave][tap pair][column block][piece][lane] x 16 bytes (csrc/conv_gbr.hip)
 *   bias_dev [N] in column order; aux_dev = x [B, r >> aux_shift, r >> aux_shift, N / 2]; mean_dev / std_dev [N / 2]
 *   out_dev  zero-bordered [B, r + 2, r + 2, N / 2] float slots, the interior is written
 * Needs r >= 16 (a power of two) and N % 128 == 0; MSR_ERR_INVALID otherwise. */
int msr_op_spade_gbr(msr_handle* h, const float* src_dev, int32_t S, const float* we_dev, const float* be_dev,
                     const float* wt_dev, const float* bias_dev, float* out_dev, int32_t B, int32_t r, int32_t N,
                     const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev, void* stream);
/* msr_op_spade_gbr in MSR_FLAG_F16_MAIN's form: the gamma|beta products are the fp16 main term alone (the fp6 cross pieces of
 * wt_dev are not read); the embedding (phase 1) is computed as in msr_op_spade_gbr.  Same arguments and checks. */
/* msr_op_spade_gbr writing the f16c6 chunk image (MSR_FLAG_CROSS_FP6's form: fp16 | fp6 e2m3 pieces with one block scale per
 * pixel and 32 channels, the input of msr_op_conv3x3_f16c with wexp_dev == NULL) into out_dev.  Same arguments and checks. */
/* Kernel-level entry of the fused head: msr_op_conv3x3_f16c with the residual epilogue on the stream kernel, whose epilogue
 * writes the head's partial sums instead of the output, then the gather kernel (synchronous).  N must be 128 and the shape the
 * stream kernel's (Cin % 128 == 0, rout >= 16 a power of two, wexp_dev given); MSR_ERR_INVALID otherwise.
 *   head_kernel_host [4, 4, 128, 1] (host), head_bias;  out_dev [B, 2 rout, 2 rout];
 *   partial_dev      optional [B, rout, rout, 32]: the partial sums, slot order as in csrc/kernels.h (HEAD_SLOTS) */
int msr_op_conv3x3_f16c_head(msr_handle* h, const float* in_dev, const float* wt_dev, const int32_t* wexp_dev,
                             const float* bias_dev, int32_t B, int32_t rout, int32_t Cin, int32_t N, const float* aux_dev,
                             int32_t aux_shift, const float* head_kernel_host, float head_bias, float* out_dev,
                             float* partial_dev, void* stream);
int msr_op_spade_gbr_f16c6(msr_handle* h, const float* src_dev, int32_t S, const float* we_dev, const float* be_dev,
                           const float* wt_dev, const float* bias_dev, float* out_dev, int32_t B, int32_t r, int32_t N,
                           const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev, void* stream);
int msr_op_spade_gbr_f16(msr_handle* h, const float* src_dev, int32_t S, const float* we_dev, const float* be_dev,
                         const float* wt_dev, const float* bias_dev, float* out_dev, int32_t B, int32_t r, int32_t N,
                         const float* aux_dev, int32_t aux_shift, const float* mean_dev, const float* std_dev, void* stream);
/* Kernel-level entry of conv_smallcin (csrc/small_kernels.hip): a 3 x 3 conv of the 2-channel source through an index map, in
 * the planner's kernel choice (tiled for Hout % 16 == 0 with >= 64 tiles, else 4 or 1 pixels per thread).
 *   src_dev   [B, S, S, 2];  w_dev HWIO [3, 3, 2, Cout] (Cout 64 | 128);  bias_dev [Cout] or NULL
 *   map       0 = encoder block 1, stride-2 SAME (S = 2 Hout);  1 = SPADE mask embedding: nearest resize of src to Hout x Hout
 *             (S a multiple of Hout), then a SAME conv
 *   act       0 none, 1 relu, 2 leaky_relu(slope)
 *   out_split 0 fp32 [.., Cout], 1 split-bf16 words, 2 split-fp16 words, 3 bf8 bytes (Cout channels in 128 bytes per pixel:
 *             32 float slots), 4 f16c chunk image;  out_padded != 0: out_dev is zero-bordered [B, Hout + 2, Hout + 2, slots]
 * Asynchronous on `stream`. */
int msr_op_conv_smallcin(msr_handle* h, const float* src_dev, int32_t S, const float* w_dev, const float* bias_dev,
                         float* out_dev, int32_t B, int32_t Hout, int32_t Cout, int32_t map, int32_t act, float slope,
                         int32_t out_split, int32_t out_padded, void* stream);
/* Kernel-level entry of norm_act: out = leaky_relu((x - mean[b]) / std[b] * gamma + beta, slope) (blocks.py:62-65).
 *   x_dev dense [B, H, W, C] (C % 4 == 0);  mean_dev / std_dev [B, C];  gamma_dev / beta_dev [C]
 *   out_padded != 0: zero-bordered [B, H + 2, W + 2, C];  out_split 1: split-bf16 words (C % 32 == 0).  Asynchronous. */
int msr_op_norm_act(msr_handle* h, const float* x_dev, const float* mean_dev, const float* std_dev, const float* gamma_dev,
                    const float* beta_dev, float* out_dev, int32_t B, int32_t H, int32_t W, int32_t C, float slope,
                    int32_t out_padded, int32_t out_split, void* stream);
/* Kernel-level entry of the dense layer, synchronous: y [B, N] = x [B, K] . W [K, N] (+ bias [N], or NULL), 1 <= B <= 16,
 * N % 4 == 0; K split and final pass as the planner launches them (the entry allocates the split-K workspace). */
int msr_op_dense(msr_handle* h, const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int32_t B,
                 int32_t K, int32_t N, void* stream);
/* Kernel-level entry of the latent sampler: mv_dev [B, 2L] = (mean | variance);  z_dev [B, L] = mean + exp(variance / 2) * eps
 * (sampler 1, eps_dev [B, L]) or mean + variance (sampler 0, eps_dev ignored).  Asynchronous. */
int msr_op_latent(msr_handle* h, const float* mv_dev, const float* eps_dev, float* z_dev, int32_t B, int32_t L,
                  int32_t sampler, void* stream);
/* Kernel-level entry of the head kernel (csrc/small_kernels.hip head_kernel), synchronous:
 *   variant 0: leaky_relu(slope) -> UpSampling2D(2) -> Conv2D(1, 4, 'same') (networks.py:54-56), kernel_host = HWIO [4,4,C,1];
 *   variant 1: Conv2DTranspose(1, 4, strides 2, 'same') -> tanh (pix2pix.py:53-57; pass slope = 1), kernel_host = [4,4,1,C]
 *   (both are [kh][kw][C] in memory).  x_dev dense [B, r, r, C] (r, C multiples of 16); out_dev [B, 2r, 2r]. */
int msr_op_head(msr_handle* h, const float* x_dev, const float* kernel_host, float bias, float* out_dev, int32_t B,
                int32_t r, int32_t C, float slope, int32_t variant, void* stream);
/* Kernel-level entry of the moments kernels (csrc/small_kernels.hip launch_moments), synchronous: per group and channel,
 *   mean_dev[g, c] = mean over p of x[g, p, c] and std_dev[g, c] = sqrtf(float(biased variance) + eps), the form every
 *   normalisation of the generator uses (G = 1: batch moments, spade.py:21; G = B: instance moments, blocks.py:63).
 *   x_dev [G, P, C] fp32 (C a multiple of 32, P >= 1, G >= 1); mean_dev / std_dev [G, C]. */
int msr_op_moments(msr_handle* h, const float* x_dev, int32_t G, int32_t P, int32_t C, float eps, float* mean_dev,
                   float* std_dev, void* stream);
/* HOST helper: the fp32 -> fp8 e4m3 (OCP "fn", round to nearest even, saturating at 448) conversion msr_load_weight
 * applies to the weights of the fp8 mode, exposed so that it can be checked against an independent implementation. */
int64_t msr_quantize_e4m3(const float* host, int64_t n, uint8_t* out);
/* Kernel-level entry of the fp8 form (MSR_FLAG_FP8) of the persistent ping-pong conv.
 *   in_dev   zero-bordered NHWC bf8 (e5m2) bytes [B, rout+2, rout+2, Cpad], Cpad = 128 or a multiple of 256 (channels beyond the real
 *            ones are zero);  wt_dev  fp8 (e4m3) bytes [9][N][Cpad];  wexp_dev [N] int32: the e8m0 exponent (127 + e,
 *            weight = byte value * 2^e) of every output channel, replicated in the word's four bytes
 *   out_mode (SPADE epilogue) 0 = fp32 [.., N/2], 1 = split-bf16 words, 3 = bf8 bytes, 128 channels or padded to a multiple of 256
 *   epilogue / aux / mean / std as msr_op_conv3x3. */
int msr_op_conv3x3_fp8(msr_handle* h, const void* in_dev, const void* wt_dev, const int32_t* wexp_dev,
                       const float* bias_dev, float* out_dev, int32_t B, int32_t rout, int32_t Cpad, int32_t N,
                       int32_t epilogue, const float* aux_dev, int32_t aux_shift, const float* mean_dev,
                       const float* std_dev, int32_t out_padded, int32_t out_mode, void* stream);
/* fp32 -> split-bf16 image: every aligned group of 32 values (one channel chunk; count % 32 == 0) becomes
 * [32 x hi bf16 | 32 x lo bf16], hi = bf16_rn(v), lo = bf16_rn(v - hi); size and addressing stay those of fp32. */
int msr_op_split_bf16(msr_handle* h, const float* in_dev, float* out_dev, int64_t count, void* stream);

/* Debug / per-block parity aid: copy a named workspace tensor of the last msr_forward to a HOST buffer
 * (names: "ws.gen.x0", "ws.gen.rb3.x1", "ws.gen.rb3.out", "ws.enc.mv", ...).  Synchronises the device.  Under a fused-head plan
 * (MSR_FLAG_FUSED_HEAD) "ws.gen.rb6.out" does not exist (MSR_ERR_INVALID, the message says so); "ws.gen.head.partial" does. */
int msr_debug_tensor(msr_handle* h, const char* name, float* host_out, int64_t count);
/* Debug, read-only: one line "<mean tensor name> <form>" per planned moments site of the network, in plan order: A (moments
 * kernels over the tensor), B (split-K epilogue), E1 | E2 (one- | two-stage finalize of conv slabs) followed by /C (slabs of
 * the conv_igemm epilogue) or /D (ping-pong / stream kernels).  NUL-terminated; MSR_ERR_INVALID when cap is too small. */
int msr_debug_moment_forms(msr_handle* h, char* out, int64_t cap);
/* Debug, read-only: one line per planned op of the network, in plan order, as "key=value" words.  kind = conv | gbr
 * (conv_gb_resident) | smallcin | norm_act | dense | latent | head | head_gather (the fused head's second launch:
 * "kind=head_gather in=ws.gen.head.partial out=output B= r=", behind a conv line with epi=5 whose mean names gen.head.wfrag) |
 * moments | moments_slabs | direct; in / wt / wexp / bias / aux
 * / mean / std / out name the op's tensors as msr_debug_tensor knows them ("input", "eps", "output": the call's own tensors,
 * "-": none); conv and gbr lines carry prec, kernel (the kernel the form names: generic | bvgpr | halo | halo16 | pp | sw on conv
 * lines, gbr on gbr lines), tile, ksplit, wt_frag, no_cross, epi, out_split, ranges (work items per pixel tile
 * of the resident kernel, else 0) and img, the weight image msr_load_weight built (F32, BF16, BF16_FRAG, F16, FP8, F16C, F16C6,
 * GBR); smallcin and norm_act lines carry out_split.  Needs a plan (after the first msr_forward or msr_forward_flops).
 * NUL-terminated; MSR_ERR_INVALID when cap is too small. */
int msr_debug_conv_forms(msr_handle* h, char* out, int64_t cap);
/* Debug, read-only: the kernel a whole-tile (no K ranges) f16c launch of msr_op_conv3x3_f16c / of the plan goes to under this
 * process's MSR_F16C_SW, by the rule that fills the forms' kernel: 1 = the stream kernel (conv_sw.hip), 0 = the ping-pong kernel.
 * cin in channels, epilogue 0 bias | 1 residual | 2 SPADE, out_mode as msr_op_conv3x3_f16c (0, 1, 4, 5). */
int msr_debug_f16c_kernel(int32_t cin, int32_t epilogue, int32_t out_mode);
/* Debug, read-only, needs NO device: the form table msr_create would build for cfg (cfg->device is not looked at) under this
 * process's environment switches, as text.  Rejects what msr_create rejects (MSR_ERR_INVALID, msr_last_error(NULL)).  One line
 * "<layer> prec= kernel= tile= ksplit= wt_frag= no_cross= img=" per conv (enc.ds2..5, gen.rb<i>.spade_<j>.gb, gen.rb<i>.conv_<j>;
 * pix2pix: p2p.down2..8, p2p.up1..7; kernel as in msr_debug_conv_forms, gbr for a gamma|beta conv that conv_gb_resident runs),
 * one line "gen.rb<i>.spade_<j> gbr= ranges= h_split= hslots= a_split= aslots=" per SPADE layer, a last line "head_fused=0|1".
 * NUL-terminated; MSR_ERR_INVALID when cap is too small (16 KB is enough). */
int msr_debug_form_table(const msr_config* cfg, char* out, int64_t cap);
/* ---- activation-range scan ------------------------------------------------------------------------ */
/* The f16c family (MSR_FLAG_F16C, _F16_MAIN, _FP8, _GB_F16X2) stores the inputs of the big convs in narrow pieces with finite
 * ranges; tests/test_gpu_conv_kernel.py::test_f16c_saturation_regimes states the three regimes of one activation a:
 *   |a| <= 448            every piece is live: the parity regime (every stated parity figure is taken here)
 *   448 < |a| <= 65504    the e4m3 cross piece clips and the conv drops to one fp16 product (2.5e-4 in that test)
 *   |a| > 65504           the producer clamps: finite and wrong
 * Keras-default weights stay near 40; trained gamma / beta need not.  The scan tells at run time which regime a call was in.
 * A record per narrow activation tensor of the plan (out_split 2 split-fp16, 3 bf8 bytes, 4 f16c, 5 f16c6; split-bf16 and fp32
 * tensors have fp32's range and are not scanned), taken on the tensor's MAIN piece hi over the interior (zero borders and zero
 * padding channels are not counted):
 *   max_abs          largest finite |hi|
 *   n_total          interior elements
 *   n_cross_clipped  format 4 only: |hi| > 464.  The boundary is 464 and not 448 because e4m3's grid around its largest value
 *                    is 416, 448, (480): under round-to-nearest-even everything up to the midpoint 464 — the tie included, 448
 *                    has the even mantissa — rounds to 448 whether or not the converter saturates; above it the saturation
 *                    changes the value.  A clipped low piece needs |hi| >= 512, so counting on hi covers it.  Format 5's block
 *                    scale follows the data: always 0
 *   n_clamped        |hi| equals the format's largest finite value (65504; bf8: 57344)
 *   n_nonfinite      hi is an infinity or a NaN */
typedef struct {
    char    tensor[48];      /* name as msr_debug_tensor knows it, e.g. "ws.gen.rb5.a1" */
    int32_t format;          /* the planner's out_split of that tensor, or MSR_RANGE_FORMAT_EMBED */
    int32_t producer;        /* index of the producing op in msr_debug_conv_forms order */
    float   max_abs;
    int64_t n_total, n_cross_clipped, n_clamped, n_nonfinite;
} msr_range_stat;
#define MSR_RANGE_FORMAT_EMBED 100
/* Asynchronous: enqueues on `stream` the zeroing of the records, ONE scan launch over every narrow activation tensor of the
 * plan (csrc/range_scan.hip) and the copy of the records to pinned host memory.  Meant to follow an msr_forward on the same
 * stream, so that it sees that call's workspace before the next call overwrites it; it is a call of its own and never part
 * of the forward's HIP graph.  One scan is outstanding per handle: a new one replaces the last.  MSR_ERR_STATE before the
 * first msr_forward.  The first scan allocates the table and the records (40 + 40 bytes per tensor). */
int msr_range_scan(msr_handle* h, void* stream);
/* Waits for the last msr_range_scan and fills up to cap records in plan order; *n = number of scanned tensors (0 for plans
 * without narrow tensors: fp32, bf16x3).  MSR_ERR_STATE if no scan was enqueued. */
int msr_range_read(msr_handle* h, msr_range_stat* out, int32_t cap, int32_t* n);
/* The embedding of a conv_gb_resident layer (kind=gbr) exists only in LDS, as fp16, and cannot be scanned.  For every gbr op,
 * in plan order: a record with format = MSR_RANGE_FORMAT_EMBED, tensor = the embedding kernel's weight name, producer = the op
 * and max_abs = max over channels c of 0.5 * sum |w[., ., ., c]| + |b_c|, from the fp32 weights the handle received — a bound
 * on |embedding| for inputs in [-0.5, 0.5] (the contract of msr_forward's in_dev); counts are 0.  Host only; needs a plan. */
int msr_range_embed_bounds(msr_handle* h, msr_range_stat* out, int32_t cap, int32_t* n);
/* Kernel-level entry of the scan, synchronous: one image in `format` (2, 3, 4, 5) holding [B, r, r, C] (C % 32 == 0),
 * zero-bordered [B, r + 2, r + 2, .] when padded != 0; chunk formats have 4 * C bytes per pixel, bf8 has C bytes padded to 128
 * or a multiple of 256.  Fills *out_stat (tensor empty, producer -1).  Bad arguments: MSR_ERR_INVALID before any allocation. */
int msr_op_range_scan(msr_handle* h, const void* img_dev, int32_t format, int32_t B, int32_t r, int32_t C, int32_t padded,
                      msr_range_stat* out_stat, void* stream);
/* ---- dirty-workspace test aids --------------------------------------------------------------------- */
/* Debug, read-only; builds the plan if the handle has none.  One line of "key=value" words per device buffer of the handle:
 *   name     the key msr_debug_tensor knows, or scratch.mom_partial | scratch.dense_partial | scratch.conv_partial |
 *            scratch.stat_ws (the raw scratch buffers that exist), or table.range_items | table.range_records |
 *            table.blend_window | table.stitch_grid
 *   kind     ws (activations, moments: keys that begin with "ws.") | scratch | weight (every other key: weight images, .wexp,
 *            folded scales) | table
 *   bytes    the size   zeroed  1 if the buffer was zero-filled when allocated   counted  1 if bytes is part of msr_device_bytes
 *            (the lines with counted=1 add up to it)
 *   r C written   zero-bordered buffers [B, r + 2, r + 2, C] only: the float slots per pixel their producer writes; the slots
 *            beyond `written` and the border stay zero and the consumer may read them.
 * NUL-terminated; MSR_ERR_INVALID when cap is too small (64 KB is enough) or an argument is null. */
int msr_debug_workspace_list(msr_handle* h, char* out, int64_t cap);
/* Debug: synchronises the device, then sets every byte of the chosen parts of the workspace to `byte` (0..255) with hipMemset /
 * hipMemset2D and synchronises again; *bytes_filled = the bytes written.  `what` is a sum of
 *   1  every kind=ws buffer with zeroed=0 and every kind=scratch buffer, in full
 *   2  the interior pixels of every zero-bordered buffer, slots 0 .. written - 1
 *   4  the border of every zero-bordered buffer, every slot (to show that the convs read it, and to restore the zeros)
 * It writes to nothing else: weights, .wexp, ws.zero_bias, the blend window, stitch_grid, the range-scan tables and whatever
 * else holds a constant, an index or an offset keep their contents, so a kernel that reads a stale word computes a wrong number
 * and never a wild address.  Captured graphs are kept.  A forward that follows must give the bits it gives on a fresh handle:
 * its result is a function of its inputs and the weights only.  MSR_ERR_INVALID for a null argument or a bad what / byte. */
int msr_debug_fill_workspace(msr_handle* h, int32_t what, int32_t byte, int64_t* bytes_filled);
/* Bytes of device memory held by the handle (weights + workspace). */
int msr_device_bytes(const msr_handle* h, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* MOONSR_H */

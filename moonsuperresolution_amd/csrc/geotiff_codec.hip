// geotiff_codec.hip — TIFF strips encoded on the device: horizontal predictor + LZW, one strip per one-wave workgroup
// (msr_lzw_encode_strips, include/moonsr.h; moonsuperresolution_amd/geotiff.py write_geotiff(encoder="device")) or one tile
// read in place from its raster per workgroup (msr_lzw_encode_blocks; write_geotiff(layout="cog", encoder="device")), either
// with the floating-point predictor instead for float32 samples (msr_tiff_encode_strips / _blocks, predictor 3), and TIFF
// strips / tiles decoded on the device: LZW, one block per one-wave workgroup (msr_lzw_decode_strips), then predictor,
// conversion to float32 and placement in the raster window, one block row per wave (msr_tiff_blocks_to_f32;
// read_geotiff(decoder="device")).
//
// Strips are compressed independently and the automaton of one strip is serial (lzw_strip.h), so the parallelism is over
// strips: a workgroup of 64 lanes takes strip blockIdx.x, blockIdx.x + gridDim.x, ...  Its dictionary is 32 KB of LDS
// (33.8 KB with the chunk buffers: four workgroups, one wave per SIMD, on a CU's 160 KB).
#include "host.h"
#include "lzw_strip.h"
#include "lzw_unstrip.h"

using namespace msr;

namespace {

__global__ __launch_bounds__(64) void lzw_encode_strips_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off,
                                                               const int32_t* __restrict__ src_len, int32_t n_strips,
                                                               int32_t sample_bytes, int32_t row_bytes, uint8_t* __restrict__ dst,
                                                               const int64_t* __restrict__ dst_off,
                                                               const int32_t* __restrict__ dst_cap, int32_t* __restrict__ dst_len) {
    __shared__ LzwWorkspace ws;
    for (int32_t s = blockIdx.x; s < n_strips; s += gridDim.x) {
        const int32_t n = src_len[s];
        int32_t len = -1;                                      // a negative length has no stream
        if (n >= 0)
            len = lzw_encode_strip(&ws, src + src_off[s], n, sample_bytes, row_bytes, dst + dst_off[s], dst_cap[s],
                                   (int)threadIdx.x, 64);
        if (threadIdx.x == 0) dst_len[s] = len;
    }
}

// The same, for blocks (tiles) read where they lie in a row-major raster: block b is block_h rows of block_w_bytes bytes whose
// valid part, blk_rows[b] rows of blk_wbytes[b] bytes at src + blk_off[b] with blk_pitch[b] bytes between rows, is read in
// place and whose padding is synthesised (lzw_fetch_block).  The pitch is per block, so tiles of several levels share a launch.
__global__ __launch_bounds__(64) void lzw_encode_blocks_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_off,
                                                               const int64_t* __restrict__ blk_pitch,
                                                               const int32_t* __restrict__ blk_wbytes,
                                                               const int32_t* __restrict__ blk_rows, int32_t n_blocks,
                                                               int32_t block_w_bytes, int32_t block_h, int32_t sample_bytes,
                                                               uint8_t* __restrict__ dst, const int64_t* __restrict__ dst_off,
                                                               const int32_t* __restrict__ dst_cap, int32_t* __restrict__ dst_len) {
    __shared__ LzwWorkspace ws;
    for (int32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const LzwBlock blk = {src + blk_off[b], blk_pitch[b], blk_wbytes[b], blk_rows[b], block_w_bytes};
        int32_t len = -1;                                      // a valid part that is not inside the block has no stream
        if (blk.valid_w_bytes >= 0 && blk.valid_w_bytes <= block_w_bytes && blk.valid_rows >= 0 && blk.valid_rows <= block_h)
            len = lzw_encode_block(&ws, blk, block_h, sample_bytes, dst + dst_off[b], dst_cap[b], (int)threadIdx.x, 64);
        if (threadIdx.x == 0) dst_len[b] = len;
    }
}

// The two kernels above with the floating-point predictor (PREDICTOR=3, float32 samples; lzw_strip.h lzw_fetch_fp) in place of
// the horizontal one.  They are kernels of their own, so the code of the two above is what it was before these existed.
__global__ __launch_bounds__(64) void tiff_encode_strips_fp_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off,
                                                                   const int32_t* __restrict__ src_len, int32_t n_strips,
                                                                   int32_t row_bytes, uint8_t* __restrict__ dst,
                                                                   const int64_t* __restrict__ dst_off,
                                                                   const int32_t* __restrict__ dst_cap, int32_t* __restrict__ dst_len) {
    __shared__ LzwWorkspace ws;
    for (int32_t s = blockIdx.x; s < n_strips; s += gridDim.x) {
        const int32_t n = src_len[s];
        int32_t len = -1;                                      // a negative length has no stream
        if (n >= 0) len = lzw_encode_strip_fp(&ws, src + src_off[s], n, row_bytes, dst + dst_off[s], dst_cap[s], (int)threadIdx.x, 64);
        if (threadIdx.x == 0) dst_len[s] = len;
    }
}

__global__ __launch_bounds__(64) void tiff_encode_blocks_fp_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_off,
                                                                   const int64_t* __restrict__ blk_pitch,
                                                                   const int32_t* __restrict__ blk_wbytes,
                                                                   const int32_t* __restrict__ blk_rows, int32_t n_blocks,
                                                                   int32_t block_w_bytes, int32_t block_h, uint8_t* __restrict__ dst,
                                                                   const int64_t* __restrict__ dst_off,
                                                                   const int32_t* __restrict__ dst_cap, int32_t* __restrict__ dst_len) {
    __shared__ LzwWorkspace ws;
    for (int32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const LzwBlock blk = {src + blk_off[b], blk_pitch[b], blk_wbytes[b], blk_rows[b], block_w_bytes};
        int32_t len = -1;                                      // a valid part that is not inside the block has no stream
        if (blk.valid_w_bytes >= 0 && blk.valid_w_bytes <= block_w_bytes && blk.valid_rows >= 0 && blk.valid_rows <= block_h)
            len = lzw_encode_block_fp(&ws, blk, block_h, dst + dst_off[b], dst_cap[b], (int)threadIdx.x, 64);
        if (threadIdx.x == 0) dst_len[b] = len;
    }
}

// The decoder's workspace is 20.9 KB of LDS (lzw_unstrip.h): seven one-wave workgroups on a CU's 160 KB.
__global__ __launch_bounds__(64) void lzw_decode_strips_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off,
                                                               const int32_t* __restrict__ src_len, int32_t n_strips,
                                                               uint8_t* __restrict__ dst, const int64_t* __restrict__ dst_off,
                                                               const int32_t* __restrict__ dst_cap, int32_t* __restrict__ dst_len) {
    __shared__ LzwDecodeWorkspace ws;
    for (int32_t s = blockIdx.x; s < n_strips; s += gridDim.x) {
        const int32_t len = lzw_decode_strip(&ws, src + src_off[s], src_len[s], dst + dst_off[s], dst_cap[s], (int)threadIdx.x, 64);
        if (threadIdx.x == 0) dst_len[s] = len;
    }
}

constexpr int PLACE_PER_LANE = 4;             // consecutive samples a lane takes: 256 per wave and step

// One wave per block row.  PREDICTOR=2 is the running sum of the row's samples modulo the sample width: each lane sums its
// PLACE_PER_LANE samples, a wave scan of the lane totals and the carry of the steps before give its start.  Unsigned addition is
// associative, so the order of the scan does not show: the bits are NumPy's cumsum on the unsigned view.
template <int SB>
__global__ __launch_bounds__(256) void tiff_blocks_to_f32_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_off,
                                                                 const int32_t* __restrict__ blk_x0, const int32_t* __restrict__ blk_y0,
                                                                 int32_t n_blocks, int32_t block_w, int32_t block_h, int32_t kind,
                                                                 int32_t predictor, float* __restrict__ out, int32_t out_row0,
                                                                 int32_t out_rows, int32_t cols) {
    const int lane = threadIdx.x & 63;
    const int64_t n_rows = (int64_t)n_blocks * block_h;
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += n_waves) {
        const int32_t b = (int32_t)(r / block_h), y = (int32_t)(r % block_h);
        const int32_t x0 = blk_x0[b], y0 = blk_y0[b];
        const int64_t row = (int64_t)y0 + y - out_row0;                      // row of the output window
        if (x0 < 0 || y0 < 0 || x0 >= cols || row < 0 || row >= out_rows) continue;
        const int32_t w = block_w < cols - x0 ? block_w : cols - x0;         // samples of this row that lie in the raster
        const uint8_t* in = src + blk_off[b] + (int64_t)y * block_w * SB;
        const bool aligned = (reinterpret_cast<uintptr_t>(in) & (SB - 1)) == 0;
        float* o = out + row * cols + x0;
        uint32_t carry = 0;
        for (int32_t j0 = 0; j0 < w; j0 += 64 * PLACE_PER_LANE) {
            const int32_t j = j0 + lane * PLACE_PER_LANE;
            uint32_t v[PLACE_PER_LANE];
#pragma unroll
            for (int i = 0; i < PLACE_PER_LANE; ++i) {
                v[i] = 0;
                if (j + i < w) {
                    const uint8_t* p = in + (int64_t)(j + i) * SB;
                    if (aligned) {
                        v[i] = SB == 4 ? *reinterpret_cast<const uint32_t*>(p) : SB == 2 ? *reinterpret_cast<const uint16_t*>(p) : *p;
                    } else {                                            // a block at an odd offset: byte by byte
#pragma unroll
                        for (int q = 0; q < SB; ++q) v[i] |= (uint32_t)p[q] << (8 * q);
                    }
                }
            }
            if (predictor == 2) {
#pragma unroll
                for (int i = 1; i < PLACE_PER_LANE; ++i) v[i] += v[i - 1];
                uint32_t incl = v[PLACE_PER_LANE - 1];
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
                    if (lane >= d) incl += up;
                }
                const uint32_t before = carry + incl - v[PLACE_PER_LANE - 1];
                carry += (uint32_t)__shfl((int)incl, 63, 64);
#pragma unroll
                for (int i = 0; i < PLACE_PER_LANE; ++i) v[i] += before;
            }
#pragma unroll
            for (int i = 0; i < PLACE_PER_LANE; ++i) {
                if (j + i >= w) continue;
                const uint32_t u = SB == 4 ? v[i] : v[i] & ((1u << (8 * (SB & 3))) - 1);
                float f;
                if (kind == 'f') f = __uint_as_float(u);
                else if (kind == 'i') f = (float)(SB == 1 ? (int32_t)(int8_t)u : SB == 2 ? (int32_t)(int16_t)u : (int32_t)u);
                else f = (float)u;
                o[j + i] = f;
            }
        }
    }
}

}  // namespace

extern "C" int msr_lzw_decode_strips(msr_handle* h, const uint8_t* src_dev, const int64_t* src_off_dev, const int32_t* src_len_dev,
                                     int32_t n_strips, uint8_t* dst_dev, const int64_t* dst_off_dev, const int32_t* dst_cap_dev,
                                     int32_t* dst_len_dev, void* stream) {
    if (!src_dev || !src_off_dev || !src_len_dev || !dst_dev || !dst_off_dev || !dst_cap_dev || !dst_len_dev)
        return fail(h, MSR_ERR_INVALID, "msr_lzw_decode_strips: null pointer");
    if (n_strips < 0) return fail(h, MSR_ERR_INVALID, "msr_lzw_decode_strips: n_strips %d < 0", n_strips);
    if (n_strips == 0) return MSR_OK;
    const int blocks = std::min<int32_t>(n_strips, 256 * 7);       // seven resident per CU
    hipLaunchKernelGGL(lzw_decode_strips_kernel, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), src_dev,
                       src_off_dev, src_len_dev, n_strips, dst_dev, dst_off_dev, dst_cap_dev, dst_len_dev);
    HIPCHK(h, hipGetLastError());
    return MSR_OK;
}

extern "C" int msr_tiff_blocks_to_f32(msr_handle* h, const uint8_t* src_dev, const int64_t* blk_off_dev, const int32_t* blk_x0_dev,
                                      const int32_t* blk_y0_dev, int32_t n_blocks, int32_t block_w, int32_t block_h,
                                      int32_t sample_kind, int32_t sample_bytes, int32_t predictor, float* out_dev,
                                      int32_t out_row0, int32_t out_rows, int32_t cols, void* stream) {
    if (!src_dev || !blk_off_dev || !blk_x0_dev || !blk_y0_dev || !out_dev)
        return fail(h, MSR_ERR_INVALID, "msr_tiff_blocks_to_f32: null pointer");
    if (n_blocks < 0) return fail(h, MSR_ERR_INVALID, "msr_tiff_blocks_to_f32: n_blocks %d < 0", n_blocks);
    if (sample_kind != 'u' && sample_kind != 'i' && sample_kind != 'f')
        return fail(h, MSR_ERR_INVALID, "msr_tiff_blocks_to_f32: sample_kind %d is not 'u', 'i' or 'f'", sample_kind);
    if ((sample_bytes != 1 && sample_bytes != 2 && sample_bytes != 4) || (sample_kind == 'f' && sample_bytes != 4))
        return fail(h, MSR_ERR_INVALID, "msr_tiff_blocks_to_f32: sample_bytes %d is not 1, 2 or 4 (4 for float samples)",
                    sample_bytes);
    if (predictor != 1 && predictor != 2)
        return fail(h, MSR_ERR_INVALID, "msr_tiff_blocks_to_f32: predictor %d is not 1 or 2", predictor);
    if (block_w <= 0 || block_h <= 0 || out_rows <= 0 || cols <= 0 || out_row0 < 0)
        return fail(h, MSR_ERR_INVALID, "msr_tiff_blocks_to_f32: geometry block %d x %d, window %d rows from %d, %d columns",
                    block_w, block_h, out_rows, out_row0, cols);
    if (n_blocks == 0) return MSR_OK;
    const int64_t n_rows = (int64_t)n_blocks * block_h;
    const int blocks = (int)std::min<int64_t>((n_rows + 3) / 4, 256 * 8 * 4);
    const hipStream_t s = static_cast<hipStream_t>(stream);
#define MSR_PLACE(SB)                                                                                                        \
    hipLaunchKernelGGL(tiff_blocks_to_f32_kernel<SB>, dim3(blocks), dim3(256), 0, s, src_dev, blk_off_dev, blk_x0_dev, blk_y0_dev, \
                       n_blocks, block_w, block_h, sample_kind, predictor, out_dev, out_row0, out_rows, cols)
    if (sample_bytes == 1) MSR_PLACE(1);
    else if (sample_bytes == 2) MSR_PLACE(2);
    else MSR_PLACE(4);
#undef MSR_PLACE
    HIPCHK(h, hipGetLastError());
    return MSR_OK;
}

// The checks and the launch of msr_lzw_encode_blocks / msr_tiff_encode_blocks, whose name `who` the messages carry.  fp: the
// floating-point predictor's kernel (sample_bytes is 4 then); else sample_bytes is msr_lzw_encode_blocks'.
static int encode_blocks(const char* who, msr_handle* h, const uint8_t* src_dev, const int64_t* blk_off_dev, const int64_t* blk_pitch_dev,
                         const int32_t* blk_wbytes_dev, const int32_t* blk_rows_dev, int32_t n_blocks, int32_t block_w_bytes,
                         int32_t block_h, int32_t sample_bytes, bool fp, uint8_t* dst_dev, const int64_t* dst_off_dev,
                         const int32_t* dst_cap_dev, int32_t* dst_len_dev, void* stream) {
    const char* null = !src_dev ? "src_dev" : !blk_off_dev ? "blk_off_dev" : !blk_pitch_dev ? "blk_pitch_dev" :
                       !blk_wbytes_dev ? "blk_wbytes_dev" : !blk_rows_dev ? "blk_rows_dev" : !dst_dev ? "dst_dev" :
                       !dst_off_dev ? "dst_off_dev" : !dst_cap_dev ? "dst_cap_dev" : !dst_len_dev ? "dst_len_dev" : nullptr;
    if (null) return fail(h, MSR_ERR_INVALID, "%s: null pointer %s", who, null);
    if (n_blocks < 0) return fail(h, MSR_ERR_INVALID, "%s: n_blocks %d < 0", who, n_blocks);
    if (sample_bytes != 0 && sample_bytes != 1 && sample_bytes != 2 && sample_bytes != 4)
        return fail(h, MSR_ERR_INVALID, "%s: sample_bytes %d is not 0, 1, 2 or 4", who, sample_bytes);
    if (block_w_bytes <= 0 || (sample_bytes && block_w_bytes % sample_bytes))
        return fail(h, MSR_ERR_INVALID, "%s: block_w_bytes %d is not a positive multiple of sample_bytes %d", who, block_w_bytes,
                    sample_bytes);
    if (block_h <= 0) return fail(h, MSR_ERR_INVALID, "%s: block_h %d <= 0", who, block_h);
    if ((int64_t)block_w_bytes * block_h > ((int64_t)1 << 30))
        return fail(h, MSR_ERR_INVALID, "%s: block_w_bytes %d x block_h %d is more than 2^30 bytes", who, block_w_bytes, block_h);
    if (n_blocks == 0) return MSR_OK;
    const int blocks = std::min<int32_t>(n_blocks, 256 * 4);       // four resident per CU, and a tile is long work: one each
    if (fp)
        hipLaunchKernelGGL(tiff_encode_blocks_fp_kernel, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), src_dev,
                           blk_off_dev, blk_pitch_dev, blk_wbytes_dev, blk_rows_dev, n_blocks, block_w_bytes, block_h, dst_dev,
                           dst_off_dev, dst_cap_dev, dst_len_dev);
    else
        hipLaunchKernelGGL(lzw_encode_blocks_kernel, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), src_dev,
                           blk_off_dev, blk_pitch_dev, blk_wbytes_dev, blk_rows_dev, n_blocks, block_w_bytes, block_h, sample_bytes,
                           dst_dev, dst_off_dev, dst_cap_dev, dst_len_dev);
    HIPCHK(h, hipGetLastError());
    return MSR_OK;
}

// The same for msr_lzw_encode_strips / msr_tiff_encode_strips.
static int encode_strips(const char* who, msr_handle* h, const uint8_t* src_dev, const int64_t* src_off_dev, const int32_t* src_len_dev,
                         int32_t n_strips, int32_t sample_bytes, bool fp, int32_t row_bytes, uint8_t* dst_dev,
                         const int64_t* dst_off_dev, const int32_t* dst_cap_dev, int32_t* dst_len_dev, void* stream) {
    if (!src_dev || !src_off_dev || !src_len_dev || !dst_dev || !dst_off_dev || !dst_cap_dev || !dst_len_dev)
        return fail(h, MSR_ERR_INVALID, "%s: null pointer", who);
    if (n_strips < 0) return fail(h, MSR_ERR_INVALID, "%s: n_strips %d < 0", who, n_strips);
    if (sample_bytes != 0 && sample_bytes != 1 && sample_bytes != 2 && sample_bytes != 4)
        return fail(h, MSR_ERR_INVALID, "%s: sample_bytes %d is not 0, 1, 2 or 4", who, sample_bytes);
    if (sample_bytes && (row_bytes <= 0 || row_bytes % sample_bytes))
        return fail(h, MSR_ERR_INVALID, "%s: row_bytes %d is not a positive multiple of sample_bytes %d", who, row_bytes,
                    sample_bytes);
    if (n_strips == 0) return MSR_OK;
    const int blocks = std::min<int32_t>(n_strips, 256 * 4 * 4);   // four resident per CU; short strips leave early
    if (fp)
        hipLaunchKernelGGL(tiff_encode_strips_fp_kernel, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), src_dev,
                           src_off_dev, src_len_dev, n_strips, row_bytes, dst_dev, dst_off_dev, dst_cap_dev, dst_len_dev);
    else
        hipLaunchKernelGGL(lzw_encode_strips_kernel, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), src_dev,
                           src_off_dev, src_len_dev, n_strips, sample_bytes, row_bytes, dst_dev, dst_off_dev, dst_cap_dev,
                           dst_len_dev);
    HIPCHK(h, hipGetLastError());
    return MSR_OK;
}

// What the two msr_tiff_encode_* entries check of their own before anything else: 0, or the failure.
static int check_predictor(const char* who, msr_handle* h, int32_t sample_bytes, int32_t predictor) {
    if (predictor != 1 && predictor != 2 && predictor != 3)
        return fail(h, MSR_ERR_INVALID, "%s: predictor %d is not 1, 2 or 3", who, predictor);
    if (sample_bytes != 1 && sample_bytes != 2 && sample_bytes != 4)
        return fail(h, MSR_ERR_INVALID, "%s: sample_bytes %d is not 1, 2 or 4", who, sample_bytes);
    if (predictor == 3 && sample_bytes != 4)
        return fail(h, MSR_ERR_INVALID, "%s: sample_bytes %d with predictor 3, which is built for 4 (float32)", who, sample_bytes);
    return MSR_OK;
}

extern "C" int msr_lzw_encode_blocks(msr_handle* h, const uint8_t* src_dev, const int64_t* blk_off_dev, const int64_t* blk_pitch_dev,
                                     const int32_t* blk_wbytes_dev, const int32_t* blk_rows_dev, int32_t n_blocks,
                                     int32_t block_w_bytes, int32_t block_h, int32_t sample_bytes, uint8_t* dst_dev,
                                     const int64_t* dst_off_dev, const int32_t* dst_cap_dev, int32_t* dst_len_dev, void* stream) {
    return encode_blocks("msr_lzw_encode_blocks", h, src_dev, blk_off_dev, blk_pitch_dev, blk_wbytes_dev, blk_rows_dev, n_blocks,
                         block_w_bytes, block_h, sample_bytes, false, dst_dev, dst_off_dev, dst_cap_dev, dst_len_dev, stream);
}

extern "C" int msr_tiff_encode_blocks(msr_handle* h, const uint8_t* src_dev, const int64_t* blk_off_dev, const int64_t* blk_pitch_dev,
                                      const int32_t* blk_wbytes_dev, const int32_t* blk_rows_dev, int32_t n_blocks,
                                      int32_t block_w_bytes, int32_t block_h, int32_t sample_bytes, int32_t predictor,
                                      uint8_t* dst_dev, const int64_t* dst_off_dev, const int32_t* dst_cap_dev, int32_t* dst_len_dev,
                                      void* stream) {
    const char* who = "msr_tiff_encode_blocks";
    if (const int rc = check_predictor(who, h, sample_bytes, predictor)) return rc;
    if (block_w_bytes <= 0 || block_w_bytes % sample_bytes)         // of the samples' width with predictor 1 as well
        return fail(h, MSR_ERR_INVALID, "%s: block_w_bytes %d is not a positive multiple of sample_bytes %d", who, block_w_bytes,
                    sample_bytes);
    return encode_blocks(who, h, src_dev, blk_off_dev, blk_pitch_dev, blk_wbytes_dev, blk_rows_dev, n_blocks, block_w_bytes,
                         block_h, predictor == 1 ? 0 : sample_bytes, predictor == 3, dst_dev, dst_off_dev, dst_cap_dev, dst_len_dev,
                         stream);
}

extern "C" int msr_lzw_encode_strips(msr_handle* h, const uint8_t* src_dev, const int64_t* src_off_dev, const int32_t* src_len_dev,
                                     int32_t n_strips, int32_t sample_bytes, int32_t row_bytes, uint8_t* dst_dev,
                                     const int64_t* dst_off_dev, const int32_t* dst_cap_dev, int32_t* dst_len_dev, void* stream) {
    return encode_strips("msr_lzw_encode_strips", h, src_dev, src_off_dev, src_len_dev, n_strips, sample_bytes, false, row_bytes,
                         dst_dev, dst_off_dev, dst_cap_dev, dst_len_dev, stream);
}

extern "C" int msr_tiff_encode_strips(msr_handle* h, const uint8_t* src_dev, const int64_t* src_off_dev, const int32_t* src_len_dev,
                                      int32_t n_strips, int32_t sample_bytes, int32_t predictor, int32_t row_bytes, uint8_t* dst_dev,
                                      const int64_t* dst_off_dev, const int32_t* dst_cap_dev, int32_t* dst_len_dev, void* stream) {
    const char* who = "msr_tiff_encode_strips";
    if (const int rc = check_predictor(who, h, sample_bytes, predictor)) return rc;
    if (row_bytes <= 0 || row_bytes % sample_bytes)                 // of the samples' width with predictor 1 as well
        return fail(h, MSR_ERR_INVALID, "%s: row_bytes %d is not a positive multiple of sample_bytes %d", who, row_bytes,
                    sample_bytes);
    return encode_strips(who, h, src_dev, src_off_dev, src_len_dev, n_strips, predictor == 1 ? 0 : sample_bytes, predictor == 3,
                         row_bytes, dst_dev, dst_off_dev, dst_cap_dev, dst_len_dev, stream);
}

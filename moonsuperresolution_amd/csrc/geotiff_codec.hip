// geotiff_codec.hip — TIFF strips encoded on the device: horizontal predictor + LZW, one strip per one-wave workgroup
// (msr_lzw_encode_strips, include/moonsr.h; moonsuperresolution_amd/geotiff.py write_geotiff(encoder="device")).
//
// Strips are compressed independently and the automaton of one strip is serial (lzw_strip.h), so the parallelism is over
// strips: a workgroup of 64 lanes takes strip blockIdx.x, blockIdx.x + gridDim.x, ...  Its dictionary is 32 KB of LDS
// (33.8 KB with the chunk buffers: four workgroups, one wave per SIMD, on a CU's 160 KB).
#include "host.h"
#include "lzw_strip.h"

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

}  // namespace

extern "C" int msr_lzw_encode_strips(msr_handle* h, const uint8_t* src_dev, const int64_t* src_off_dev, const int32_t* src_len_dev,
                                     int32_t n_strips, int32_t sample_bytes, int32_t row_bytes, uint8_t* dst_dev,
                                     const int64_t* dst_off_dev, const int32_t* dst_cap_dev, int32_t* dst_len_dev, void* stream) {
    if (!src_dev || !src_off_dev || !src_len_dev || !dst_dev || !dst_off_dev || !dst_cap_dev || !dst_len_dev)
        return fail(h, MSR_ERR_INVALID, "msr_lzw_encode_strips: null pointer");
    if (n_strips < 0) return fail(h, MSR_ERR_INVALID, "msr_lzw_encode_strips: n_strips %d < 0", n_strips);
    if (sample_bytes != 0 && sample_bytes != 1 && sample_bytes != 2 && sample_bytes != 4)
        return fail(h, MSR_ERR_INVALID, "msr_lzw_encode_strips: sample_bytes %d is not 0, 1, 2 or 4", sample_bytes);
    if (sample_bytes && (row_bytes <= 0 || row_bytes % sample_bytes))
        return fail(h, MSR_ERR_INVALID, "msr_lzw_encode_strips: row_bytes %d is not a positive multiple of sample_bytes %d",
                    row_bytes, sample_bytes);
    if (n_strips == 0) return MSR_OK;
    const int blocks = std::min<int32_t>(n_strips, 256 * 4 * 4);   // four resident per CU; short strips leave early
    hipLaunchKernelGGL(lzw_encode_strips_kernel, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), src_dev,
                       src_off_dev, src_len_dev, n_strips, sample_bytes, row_bytes, dst_dev, dst_off_dev, dst_cap_dev,
                       dst_len_dev);
    HIPCHK(h, hipGetLastError());
    return MSR_OK;
}

// tiff_overview.hip — one reduced-resolution level of a raster on the device (msr_overview_half, include/moonsr.h;
// moonsuperresolution_amd/geotiff.py write_geotiff(tile=, overviews=, encoder="device")).  The rule is tiff_overview.h's; the
// kernel is one thread per destination pixel, consecutive lanes on consecutive destination columns, so a wave reads 128
// consecutive source samples of each of two rows and writes 64 consecutive ones.  Streaming: no LDS, nothing is reused.
#include "host.h"
#include "tiff_overview.h"

using namespace msr;

namespace {

constexpr int OVERVIEW_BLOCK = 256;

template <typename T>
__global__ __launch_bounds__(OVERVIEW_BLOCK) void overview_half_kernel(const T* __restrict__ src, int32_t rows, int32_t cols,
                                                                      int32_t dst_rows, int32_t dst_cols, int32_t has_nodata,
                                                                      float no_value, T* __restrict__ dst) {
    const int64_t j = (int64_t)blockIdx.x * OVERVIEW_BLOCK + threadIdx.x;
    if (j >= dst_cols) return;
    for (int32_t i = blockIdx.y; i < dst_rows; i += gridDim.y)
        dst[(int64_t)i * dst_cols + j] = overview_pixel<T>(src, rows, cols, i, (int32_t)j, has_nodata != 0, no_value);
}

}  // namespace

extern "C" int msr_overview_half(msr_handle* h, const void* src_dev, int32_t rows, int32_t cols, int32_t sample_kind,
                                 int32_t sample_bytes, int32_t has_nodata, float no_value, void* dst_dev, void* stream) {
    if (const char* bad = overview_bad_argument(src_dev, rows, cols, sample_kind, sample_bytes, has_nodata, dst_dev))
        return fail(h, MSR_ERR_INVALID, "msr_overview_half: bad argument %s", bad);
    const int32_t dst_rows = (rows + 1) / 2, dst_cols = (cols + 1) / 2;
    const dim3 grid((dst_cols + OVERVIEW_BLOCK - 1) / OVERVIEW_BLOCK, std::min<int32_t>(dst_rows, 65535));
    const hipStream_t s = static_cast<hipStream_t>(stream);
#define MSR_OVERVIEW(T)                                                                                                      \
    hipLaunchKernelGGL(overview_half_kernel<T>, grid, dim3(OVERVIEW_BLOCK), 0, s, static_cast<const T*>(src_dev), rows, cols, \
                       dst_rows, dst_cols, has_nodata, no_value, static_cast<T*>(dst_dev))
    if (sample_kind == 'f') MSR_OVERVIEW(float);
    else if (sample_bytes == 2) MSR_OVERVIEW(uint16_t);
    else MSR_OVERVIEW(uint8_t);
#undef MSR_OVERVIEW
    HIPCHK(h, hipGetLastError());
    return MSR_OK;
}

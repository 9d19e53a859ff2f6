// Host-only unit of libmoonsr_hip.so (no device code): the overview rule of the device writer (tiff_overview.h) looped over
// host buffers, so that the CPU suite and tools/overview_check.cpp can hold it against the NumPy twin without a GPU.  Compiled
// with -ffp-contract=off like the device units.
#include "../../include/moonsr.h"
#include "tiff_overview.h"

namespace {

template <typename T>
void overview_half(const void* src, int32_t rows, int32_t cols, bool has_nodata, float no_value, void* dst) {
    const int32_t dst_rows = (rows + 1) / 2, dst_cols = (cols + 1) / 2;
    for (int32_t i = 0; i < dst_rows; ++i)
        for (int32_t j = 0; j < dst_cols; ++j)
            static_cast<T*>(dst)[(int64_t)i * dst_cols + j] =
                msr::overview_pixel<T>(static_cast<const T*>(src), rows, cols, i, j, has_nodata, no_value);
}

}  // namespace

extern "C" int msr_overview_half_host(const void* src, int32_t rows, int32_t cols, int32_t sample_kind, int32_t sample_bytes,
                                      int32_t has_nodata, float no_value, void* dst) {
    if (msr::overview_bad_argument(src, rows, cols, sample_kind, sample_bytes, has_nodata, dst)) return -1;
    if (sample_kind == 'f') overview_half<float>(src, rows, cols, has_nodata != 0, no_value, dst);
    else if (sample_bytes == 2) overview_half<uint16_t>(src, rows, cols, false, 0.0f, dst);
    else overview_half<uint8_t>(src, rows, cols, false, 0.0f, dst);
    return 0;
}

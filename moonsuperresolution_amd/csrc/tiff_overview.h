// tiff_overview.h — ONE pixel of a reduced-resolution level (a TIFF overview) as a __host__ __device__ function, in the manner
// of infill_solve.h: the kernel of tiff_overview.hip runs it with one thread per destination pixel, msr_overview_half_host
// (host_overview.cpp) and tools/overview_check.cpp loop it on the host, and moonsuperresolution_amd/geotiff.py::
// overview_reference is the NumPy twin whose bits it reproduces.
//
// dst is ceil(rows / 2) x ceil(cols / 2); dst[i][j] comes from the block src[2i : 2i + 2][2j : 2j + 2] clipped to the raster
// (a 1 x 2, 2 x 1 or 1 x 1 block at the last row / column of an odd shape).
//   float32     a pixel COUNTS iff v != no_value (a NaN counts and propagates; without nodata every pixel counts).  With no
//               counting pixel the result is no_value.  Otherwise it is s / (float)n: s the float32 sum of the n counting values
//               in row-major order, STARTED FROM THE FIRST of them, not from 0 (so that -0.0 alone stays -0.0), one rounding per
//               addition and one for the division (the units that include this compile with -ffp-contract=off; there is no
//               product to contract, the flag keeps it so).
//   uint8 / 16  the maximum of the block: the overview of `good` is 1 exactly where the overview of `mean` is not nodata.
// Every read is behind a bounds test on the row and the column; offsets are 64-bit (a product is 4.2 GB).
#pragma once
#include <stdint.h>

#include <type_traits>

#if defined(__HIPCC__)
#define OVERVIEW_HD __host__ __device__
#else
#define OVERVIEW_HD
#endif

namespace msr {

// dst[i][j] of the level below src [rows][cols]; 0 <= i < ceil(rows / 2), 0 <= j < ceil(cols / 2).  T is float, uint8_t or
// uint16_t; has_nodata / no_value are looked at for float only.
template <typename T>
OVERVIEW_HD inline T overview_pixel(const T* src, int32_t rows, int32_t cols, int32_t i, int32_t j, bool has_nodata, float no_value) {
    const int32_t r0 = 2 * i, c0 = 2 * j;
    if constexpr (std::is_same<T, float>::value) {
        float s = 0.0f;
        int n = 0;
        for (int k = 0; k < 4; ++k) {                      // row-major: (0,0) (0,1) (1,0) (1,1)
            const int32_t r = r0 + (k >> 1), c = c0 + (k & 1);
            if (r >= rows || c >= cols) continue;
            const float v = src[(int64_t)r * cols + c];
            if (has_nodata && !(v != no_value)) continue;
            s = n ? s + v : v;
            ++n;
        }
        return n ? s / (float)n : no_value;
    } else {
        T m = 0;
        for (int k = 0; k < 4; ++k) {
            const int32_t r = r0 + (k >> 1), c = c0 + (k & 1);
            if (r >= rows || c >= cols) continue;
            const T v = src[(int64_t)r * cols + c];
            m = v > m ? v : m;
        }
        return m;
    }
}

// The argument checks the device and the host entry share: nullptr if the arguments are fine, else the name of the first bad one.
inline const char* overview_bad_argument(const void* src, int32_t rows, int32_t cols, int32_t sample_kind, int32_t sample_bytes,
                                         int32_t has_nodata, const void* dst) {
    if (!src) return "src (null pointer)";
    if (!dst) return "dst (null pointer)";
    if (rows <= 0) return "rows (<= 0)";
    if (cols <= 0) return "cols (<= 0)";
    if ((int64_t)rows * cols > INT32_MAX) return "rows x cols (more than 2^31 - 1 source pixels)";
    if (sample_kind != 'f' && sample_kind != 'u') return "sample_kind (not 'f' or 'u')";
    if (sample_kind == 'f' ? sample_bytes != 4 : (sample_bytes != 1 && sample_bytes != 2))
        return "sample_bytes (4 for 'f', 1 or 2 for 'u')";
    if (has_nodata != 0 && has_nodata != 1) return "has_nodata (not 0 or 1)";
    if (has_nodata && sample_kind != 'f') return "has_nodata (set with an integer sample_kind)";
    return nullptr;
}

}  // namespace msr

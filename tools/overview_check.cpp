// CPU only, stand-alone: the overview rule of the device writer (csrc/tiff_overview.h, looped by msr_overview_half_host) under
// AddressSanitizer / UBSan, against a plain re-statement written here: gather the block's pixels that lie in the raster into
// a list in row-major order, drop the no-data ones, fold.  Source and destination are heap blocks of exactly their size, so a
// read or write outside either is an error.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Imoonsuperresolution_amd/csrc tools/overview_check.cpp moonsuperresolution_amd/csrc/host_overview.cpp \
//       -o /tmp/overview_check && /tmp/overview_check
// Cases: every shape 1 .. 9 x 1 .. 9 and 300 random ones up to 70 x 130 (odd rows and columns, one row, one column), float32
// with and without no-data (half the pixels no-data, some NaN, some +-0) and uint8 / uint16; the entry's refusals.  Compared
// bit for bit.
#include "tiff_overview.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
extern "C" int msr_overview_half_host(const void* src, int32_t rows, int32_t cols, int32_t sample_kind, int32_t sample_bytes,
                                      int32_t has_nodata, float no_value, void* dst);
static const float NV = -32768.f;
static int n_cases = 0, n_failed = 0;

template <typename T>
static T plain(const T* src, int rows, int cols, int i, int j, bool has_nodata) {
    std::vector<T> v;
    for (int r = 2 * i; r < 2 * i + 2 && r < rows; ++r)
        for (int c = 2 * j; c < 2 * j + 2 && c < cols; ++c) v.push_back(src[(size_t)r * cols + c]);
    if constexpr (std::is_same<T, float>::value) {
        std::vector<float> w;
        for (float x : v)
            if (!has_nodata || x != NV) w.push_back(x);
        if (w.empty()) return NV;
        volatile float s = w[0];                         // volatile: one float32 rounding per step, whatever the compiler likes
        for (size_t k = 1; k < w.size(); ++k) s = s + w[k];
        volatile float n = (float)w.size();
        return s / n;
    } else {
        T m = 0;
        for (T x : v) m = x > m ? x : m;
        return m;
    }
}

template <typename T>
static void check(int rows, int cols, bool has_nodata, std::mt19937& rng) {
    const int dr = (rows + 1) / 2, dc = (cols + 1) / 2;
    T* src = (T*)malloc(sizeof(T) * rows * cols);
    T* dst = (T*)malloc(sizeof(T) * dr * dc);
    for (int k = 0; k < rows * cols; ++k) {
        if constexpr (std::is_same<T, float>::value) {
            const unsigned u = rng() % 100;
            const float mag[4] = {1e-3f, 1.f, 1e4f, 1e8f};
            src[k] = u < 45 ? NV : u < 50 ? NAN : u < 54 ? 0.f : u < 58 ? -0.f : ((int)(rng() % 2001) - 1000) * mag[rng() % 4] / 7.f;
        } else {
            src[k] = (T)(rng() % 3 ? rng() : 0);
        }
    }
    memset(dst, 0x5A, sizeof(T) * dr * dc);
    const bool f = std::is_same<T, float>::value;
    const int rc = msr_overview_half_host(src, rows, cols, f ? 'f' : 'u', (int)sizeof(T), has_nodata, NV, dst);
    bool ok = rc == 0;
    for (int i = 0; i < dr && ok; ++i)
        for (int j = 0; j < dc && ok; ++j) {
            const T want = plain<T>(src, rows, cols, i, j, has_nodata);
            ok = memcmp(&want, &dst[(size_t)i * dc + j], sizeof(T)) == 0;
            if (!ok) printf("FAIL %d x %d %s nodata %d at (%d, %d)\n", rows, cols, f ? "f32" : sizeof(T) == 2 ? "u16" : "u8", has_nodata, i, j);
        }
    ++n_cases;
    n_failed += !ok;
    free(src);
    free(dst);
}

static void check_all(int rows, int cols, std::mt19937& rng) {
    check<float>(rows, cols, true, rng);
    check<float>(rows, cols, false, rng);
    check<uint8_t>(rows, cols, false, rng);
    check<uint16_t>(rows, cols, false, rng);
}

int main() {
    std::mt19937 rng(20240611);
    for (int r = 1; r <= 9; ++r)
        for (int c = 1; c <= 9; ++c) check_all(r, c, rng);
    for (int k = 0; k < 300; ++k) check_all(1 + rng() % 70, 1 + rng() % 130, rng);
    check_all(1, 257, rng);
    check_all(257, 1, rng);
    {   // the refusals: nothing is read or written
        float a[4] = {1, 2, 3, 4}, d[1] = {0};
        int ok = msr_overview_half_host(a, 2, 2, 'f', 4, 1, NV, d) == 0 && d[0] == 2.5f;
        ok &= msr_overview_half_host(nullptr, 2, 2, 'f', 4, 1, NV, d) == -1;
        ok &= msr_overview_half_host(a, 2, 2, 'f', 4, 1, NV, nullptr) == -1;
        ok &= msr_overview_half_host(a, 0, 2, 'f', 4, 1, NV, d) == -1;
        ok &= msr_overview_half_host(a, 2, -1, 'f', 4, 1, NV, d) == -1;
        ok &= msr_overview_half_host(a, 65536, 32768, 'f', 4, 1, NV, d) == -1;
        ok &= msr_overview_half_host(a, 2, 2, 'i', 4, 0, NV, d) == -1;
        ok &= msr_overview_half_host(a, 2, 2, 'f', 2, 0, NV, d) == -1;
        ok &= msr_overview_half_host(a, 2, 2, 'u', 4, 0, NV, d) == -1;
        ok &= msr_overview_half_host(a, 2, 2, 'u', 2, 1, NV, d) == -1;
        ok &= msr_overview_half_host(a, 2, 2, 'f', 4, 2, NV, d) == -1;
        ++n_cases;
        n_failed += !ok;
        if (!ok) printf("FAIL refusals\n");
    }
    printf("%d cases, %d failed\n", n_cases, n_failed);
    return n_failed ? 1 : 0;
}

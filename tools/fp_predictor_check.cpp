// CPU only, stand-alone: the floating-point predictor (PREDICTOR=3) of the device GeoTIFF encoder (csrc/lzw_strip.h: lzw_fetch_fp
// + the automaton, run here with one lane: lzw_encode_strip_fp directly, lzw_encode_block_fp through msr_tiff_encode_block_host)
// under AddressSanitizer / UBSan, against msr_lzw_encode of the bytes built by a plain re-statement written here: pad, regroup
// every row into four planes with the most significant bytes first, difference the regrouped row from its end.  Every source
// is a heap block that ends with the last byte the encoder may read and every slot one of exactly the stream's length, so a
// read or write outside either is an error.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Imoonsuperresolution_amd/csrc \
//       tools/fp_predictor_check.cpp moonsuperresolution_amd/csrc/host_codecs.cpp -o /tmp/fp_predictor_check \
//       && /tmp/fp_predictor_check
// Cases.  Strips: three rows of 33, 64, 65, 257 and 16400 samples (planes shorter than a chunk of 256 bytes, a row of exactly
// one chunk, planes longer than a chunk, rows over 64 KiB); 17 rows of 33 samples in strips of 5 rows (the last one shorter); 0
// rows; each from a source on a 4-byte boundary (aligned 32-bit loads) and 1, 2 and 3 bytes off it (byte loads).  Blocks of
// 16 x 16, 32 x 48 and 48 x 32 samples with a valid part of 1 x 1, everything, 17 columns, 0 rows, 0 columns, one row that is
// the last of its raster; a pitch equal to the valid width, larger, and no multiple of 4; terrain-like samples, random bytes
// (the table fills and is cleared) and one value.  A slot one byte short.  Predictors 1 and 2 of msr_tiff_encode_block_host
// against msr_lzw_encode_block_host.  The refusals.  Compared byte for byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "lzw_strip.h"

extern "C" int64_t msr_lzw_encode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);
extern "C" int64_t msr_lzw_encode_block_host(const uint8_t* src, int64_t pitch, int32_t valid_w_bytes, int32_t valid_rows,
                                             int32_t block_w_bytes, int32_t block_h, int32_t sample_bytes, uint8_t* dst, int64_t cap);
extern "C" int64_t msr_tiff_encode_block_host(const uint8_t* src, int64_t pitch, int32_t valid_w_bytes, int32_t valid_rows,
                                              int32_t block_w_bytes, int32_t block_h, int32_t sample_bytes, int32_t predictor,
                                              uint8_t* dst, int64_t cap);
static msr::LzwWorkspace ws;
static int n_cases = 0, n_failed = 0;

// kind 0: float32 terrain (a random walk in quarter metres around -2000), 1: random bytes, 2: one value
static void fill(uint8_t* p, size_t n, int kind, std::mt19937& rng) {
    float walk = -2000.0f;
    for (size_t i = 0; i < n; ++i) {
        if (i % 4 == 0) walk += 0.25f * (float)((int)(rng() % 7) - 3);
        uint8_t b[4];
        memcpy(b, &walk, 4);
        p[i] = kind == 1 ? (uint8_t)rng() : kind == 2 ? 7 : b[i % 4];
    }
}

// rows x row_bytes bytes of float32 samples, in place: the predictor's bytes
static void twin(std::vector<uint8_t>& blk, int rows, int row_bytes) {
    const int w = row_bytes / 4;
    std::vector<uint8_t> t(row_bytes);
    for (int y = 0; y < rows; ++y) {
        uint8_t* row = &blk[(size_t)y * row_bytes];
        for (int p = 0; p < 4; ++p)
            for (int x = 0; x < w; ++x) t[(size_t)p * w + x] = row[4 * x + 3 - p];
        for (int q = row_bytes - 1; q > 0; --q) t[q] = (uint8_t)(t[q] - t[q - 1]);
        if (row_bytes) memcpy(row, t.data(), row_bytes);
    }
}

static std::vector<uint8_t> reference(const std::vector<uint8_t>& bytes) {
    std::vector<uint8_t> want(bytes.size() + bytes.size() / 2 + 1024);
    uint8_t dummy = 0;
    const int64_t n = msr_lzw_encode(bytes.size() ? bytes.data() : &dummy, (int64_t)bytes.size(), want.data(), (int64_t)want.size());
    want.resize(n > 0 ? n : 0);
    return want;
}

static void report(bool ok, const char* what, int a, int b, int c, int d, long long e, int kind) {
    if (!ok) printf("FAIL %s %d %d %d %d %lld kind %d\n", what, a, b, c, d, e, kind);
    ++n_cases;
    n_failed += !ok;
}

// a strip of `rows` rows of w samples that begins `shift` bytes behind a 4-byte boundary
static void check_strip(int rows, int w, int shift, int kind, std::mt19937& rng) {
    const int row_bytes = 4 * w;
    const size_t n = (size_t)rows * row_bytes;
    uint8_t* heap = (uint8_t*)malloc(n + shift ? n + shift : 1);      // ends with the strip's last byte
    uint8_t* src = heap + shift;
    fill(src, n, kind, rng);
    std::vector<uint8_t> bytes(src, src + n);
    twin(bytes, rows, row_bytes);
    const std::vector<uint8_t> want = reference(bytes);
    const int32_t len = (int32_t)want.size();
    bool ok = len > 0;
    if (ok) {
        uint8_t* dst = (uint8_t*)malloc(len);
        ok = msr::lzw_encode_strip_fp(&ws, src, (int32_t)n, row_bytes, dst, len, 0, 1) == len && memcmp(dst, want.data(), len) == 0;
        ok = ok && msr::lzw_encode_strip_fp(&ws, src, (int32_t)n, row_bytes, dst, len - 1, 0, 1) == -1;
        free(dst);
    }
    report(ok, "strip rows w shift", rows, w, shift, 0, 0, kind);
    free(heap);
}

// a block of bh rows of bw samples whose valid part is vr rows of vw samples at `pitch` bytes, `shift` bytes behind a boundary
static void check_block(int bh, int bw, int vr, int vw, int64_t pitch, int shift, int kind, std::mt19937& rng) {
    const int bwb = 4 * bw, vwb = 4 * vw;
    const size_t n_src = vr > 0 && vwb > 0 ? (size_t)(vr - 1) * pitch + vwb : 0;
    uint8_t* heap = (uint8_t*)malloc(n_src + shift ? n_src + shift : 1);
    uint8_t* src = heap + shift;                                // ends with the last valid byte
    fill(src, n_src, kind, rng);
    std::vector<uint8_t> blk((size_t)bwb * bh, 0);
    for (int y = 0; y < vr; ++y) memcpy(&blk[(size_t)y * bwb], src + y * pitch, vwb);
    twin(blk, bh, bwb);
    const std::vector<uint8_t> want = reference(blk);
    const int64_t len = (int64_t)want.size();
    bool ok = len > 0;
    if (ok) {
        uint8_t* dst = (uint8_t*)malloc(len);
        ok = msr_tiff_encode_block_host(src, pitch, vwb, vr, bwb, bh, 4, 3, dst, len) == len && memcmp(dst, want.data(), len) == 0;
        ok = ok && msr_tiff_encode_block_host(src, pitch, vwb, vr, bwb, bh, 4, 3, dst, len - 1) == -1;
        free(dst);
    }
    report(ok, "block bh bw vr vw pitch", bh, bw, vr, vw, (long long)pitch, kind);
    free(heap);
}

// predictors 1 and 2 of the new host entry are the old one's streams
static void check_old(int sb, std::mt19937& rng) {
    const int bwb = 96, bh = 16, vwb = 96 - sb, vr = 15;
    const int64_t pitch = vwb + 5 * sb;
    std::vector<uint8_t> src((size_t)(vr - 1) * pitch + vwb);
    fill(src.data(), src.size(), 0, rng);
    std::vector<uint8_t> a(4096), b(4096);
    bool ok = true;
    for (int predictor = 1; predictor <= 2; ++predictor) {
        const int64_t na = msr_lzw_encode_block_host(src.data(), pitch, vwb, vr, bwb, bh, predictor == 2 ? sb : 0, a.data(), 4096);
        const int64_t nb = msr_tiff_encode_block_host(src.data(), pitch, vwb, vr, bwb, bh, sb, predictor, b.data(), 4096);
        ok = ok && na > 0 && na == nb && memcmp(a.data(), b.data(), na) == 0;
    }
    report(ok, "old and new entry sb", sb, 0, 0, 0, 0, 0);
}

int main() {
    std::mt19937 rng(20241021);
    for (int w : {33, 64, 65, 257, 16400})
        for (int shift = 0; shift < 4; ++shift) check_strip(3, w, shift, 0, rng);
    for (int rows : {5, 2, 17, 0, 1})
        for (int shift : {0, 3}) check_strip(rows, 33, shift, 0, rng);
    check_strip(48, 48, 0, 1, rng);
    check_strip(48, 48, 1, 1, rng);
    check_strip(20, 10, 0, 2, rng);
    check_strip(1, 1, 2, 0, rng);
    const int shapes[3][2] = {{16, 16}, {32, 48}, {48, 32}};
    for (const auto& s : shapes) {
        const int bh = s[0], bw = s[1];
        const int parts[6][2] = {{1, 1}, {bh, bw}, {bh, bw > 17 ? 17 : 9}, {0, bw}, {bh, 0}, {1, bw}};
        for (const auto& v : parts) {
            const int vr = v[0], vw = v[1];
            for (int kind = 0; kind < 3; ++kind) {
                check_block(bh, bw, vr, vw, 4 * vw, 0, kind, rng);                 // tight
                check_block(bh, bw, vr, vw, 4 * vw + 20, 0, kind, rng);            // a raster's pitch
                check_block(bh, bw, vr, vw, 4 * vw + 20, 2, kind, rng);            // off the boundary
                check_block(bh, bw, vr, vw, 4 * vw + 7, 0, kind, rng);             // rows off the boundary
            }
        }
    }
    check_block(48, 48, 47, 47, 1 << 20, 0, 1, rng);
    for (int sb : {1, 2, 4}) check_old(sb, rng);
    {   // the refusals: nothing is read or written
        uint8_t s[256] = {0}, d[2048];
        int ok = msr_tiff_encode_block_host(s, 16, 16, 8, 16, 8, 4, 3, d, 2048) > 0;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 8, 16, 8, 4, 0, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 8, 16, 8, 4, 4, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 8, 16, 8, 2, 3, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 8, 16, 8, 1, 3, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 8, 16, 8, 0, 1, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 8, 16, 8, 3, 2, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 18, 18, 8, 18, 8, 4, 3, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 18, 18, 8, 18, 8, 4, 1, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(nullptr, 16, 16, 8, 16, 8, 4, 3, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 8, 16, 8, 4, 3, nullptr, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 8, 16, 8, 4, 3, d, -1) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 20, 8, 16, 8, 4, 3, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 9, 16, 8, 4, 3, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 8, 16, 0, 4, 3, d, 2048) == -1;
        ok &= msr_tiff_encode_block_host(s, 16, 16, 8, 1 << 16, 1 << 15, 4, 3, d, 2048) == -1;
        report(ok, "refusals", 0, 0, 0, 0, 0, 0);
    }
    printf("%d cases, %d failed\n", n_cases, n_failed);
    return n_failed ? 1 : 0;
}

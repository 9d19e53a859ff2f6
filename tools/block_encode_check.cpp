// CPU only, stand-alone: the in-place block encoder of the device writer (csrc/lzw_strip.h: lzw_fetch_block + the automaton,
// run with one lane by msr_lzw_encode_block_host) under AddressSanitizer / UBSan, against msr_lzw_encode of the block built
// by a plain re-statement written here: copy the valid part into a zero block, then difference every block row from its end.
// The source is a heap block that ends with the block's last valid byte and the slot one of exactly the stream's length, so
// a read or write outside either is an error.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Imoonsuperresolution_amd/csrc \
//       tools/block_encode_check.cpp moonsuperresolution_amd/csrc/host_codecs.cpp -o /tmp/block_encode_check \
//       && /tmp/block_encode_check
// Cases: sample bytes 0 / 1 / 2 / 4; block rows of 16, 64, 96, 256 and 320 bytes; 16 and 48 block rows; a valid width of one
// sample, all but one and all; 1, block_h - 1 and block_h valid rows; a pitch equal to the valid width, larger, and (1-byte
// samples) odd; a 48 x 48 float32 block of random bytes (the table fills and is cleared); constant blocks; a slot one byte
// short; the entry's refusals.  Compared byte for byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
extern "C" int64_t msr_lzw_encode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);
extern "C" int64_t msr_lzw_encode_block_host(const uint8_t* src, int64_t pitch, int32_t valid_w_bytes, int32_t valid_rows,
                                             int32_t block_w_bytes, int32_t block_h, int32_t sample_bytes, uint8_t* dst, int64_t cap);
static int n_cases = 0, n_failed = 0;

// kind 0: a random walk of samples (rows difference to bytes that repeat), 1: random bytes, 2: one value
static void check(int sb, int bw, int bh, int vw, int vr, int64_t pitch, int kind, std::mt19937& rng) {
    const int unit = sb ? sb : 1;
    const size_t n_src = (size_t)(vr - 1) * pitch + vw;
    uint8_t* src = (uint8_t*)malloc(n_src);
    uint32_t walk = 1000;
    for (size_t i = 0; i < n_src; ++i) {
        if (i % unit == 0) walk += (int)(rng() % 7) - 3;
        src[i] = kind == 1 ? (uint8_t)rng() : kind == 2 ? 7 : (uint8_t)(walk >> (8 * (i % unit)));
    }
    std::vector<uint8_t> blk((size_t)bw * bh, 0);
    for (int y = 0; y < vr; ++y) memcpy(&blk[(size_t)y * bw], src + y * pitch, vw);
    if (sb)
        for (int y = 0; y < bh; ++y)
            for (int j = bw / sb - 1; j > 0; --j) {              // from the row's end, so that each sample still sees its neighbour
                uint32_t cur = 0, prev = 0;
                memcpy(&cur, &blk[(size_t)y * bw + j * sb], sb);
                memcpy(&prev, &blk[(size_t)y * bw + (j - 1) * sb], sb);
                cur -= prev;
                memcpy(&blk[(size_t)y * bw + j * sb], &cur, sb);
            }
    std::vector<uint8_t> want(blk.size() + blk.size() / 2 + 1024);
    const int64_t n = msr_lzw_encode(blk.data(), (int64_t)blk.size(), want.data(), (int64_t)want.size());
    bool ok = n > 0;
    if (ok) {
        uint8_t* dst = (uint8_t*)malloc(n);
        ok = msr_lzw_encode_block_host(src, pitch, vw, vr, bw, bh, sb, dst, n) == n && memcmp(dst, want.data(), n) == 0;
        ok = ok && msr_lzw_encode_block_host(src, pitch, vw, vr, bw, bh, sb, dst, n - 1) == -1;
        free(dst);
    }
    if (!ok) printf("FAIL sb %d block %d x %d valid %d x %d pitch %lld kind %d\n", sb, bw, bh, vw, vr, (long long)pitch, kind);
    ++n_cases;
    n_failed += !ok;
    free(src);
}

int main() {
    std::mt19937 rng(20240920);
    const int sbs[4] = {0, 1, 2, 4}, bws[5] = {16, 64, 96, 256, 320}, bhs[2] = {16, 48};
    for (int sb : sbs)
        for (int bw : bws)
            for (int bh : bhs) {
                const int unit = sb ? sb : 1;
                const int vws[3] = {unit, bw - unit, bw}, vrs[3] = {1, bh - 1, bh};
                for (int vw : vws)
                    for (int vr : vrs) {
                        check(sb, bw, bh, vw, vr, vw, 0, rng);
                        check(sb, bw, bh, vw, vr, vw + 5 * unit, 0, rng);
                        if (unit == 1) check(sb, bw, bh, vw, vr, (vw + 8) | 1, 0, rng);
                        check(sb, bw, bh, vw, vr, vw + 3 * unit, 2, rng);
                    }
            }
    check(4, 192, 48, 192, 48, 192, 1, rng);
    check(0, 192, 48, 192, 48, 192, 1, rng);
    check(4, 192, 48, 188, 47, 1 << 20, 1, rng);                 // a raster's pitch
    {   // the refusals: nothing is read or written
        uint8_t s[64] = {0}, d[2048];
        int ok = msr_lzw_encode_block_host(s, 8, 8, 8, 8, 8, 1, d, 2048) > 0;
        ok &= msr_lzw_encode_block_host(nullptr, 8, 8, 8, 8, 8, 1, d, 2048) == -1;
        ok &= msr_lzw_encode_block_host(s, 8, 8, 8, 8, 8, 1, nullptr, 2048) == -1;
        ok &= msr_lzw_encode_block_host(s, 8, 8, 8, 8, 8, 1, d, -1) == -1;
        ok &= msr_lzw_encode_block_host(s, 8, 8, 8, 8, 8, 3, d, 2048) == -1;
        ok &= msr_lzw_encode_block_host(s, 8, 8, 8, 0, 8, 1, d, 2048) == -1;
        ok &= msr_lzw_encode_block_host(s, 8, 8, 8, 8, 0, 1, d, 2048) == -1;
        ok &= msr_lzw_encode_block_host(s, 8, 6, 8, 6, 8, 4, d, 2048) == -1;
        ok &= msr_lzw_encode_block_host(s, 8, 9, 8, 8, 8, 1, d, 2048) == -1;
        ok &= msr_lzw_encode_block_host(s, 8, 8, 9, 8, 8, 1, d, 2048) == -1;
        ok &= msr_lzw_encode_block_host(s, 8, 8, 8, 1 << 16, 1 << 15, 1, d, 2048) == -1;
        ++n_cases;
        n_failed += !ok;
        if (!ok) printf("FAIL refusals\n");
    }
    printf("%d cases, %d failed\n", n_cases, n_failed);
    return n_failed ? 1 : 0;
}
